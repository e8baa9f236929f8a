"""Block-granular autograd Functions of the CenterNet/CornerNet ResNet training path.

Each Function runs one reference module group entirely on libscdhip kernels:
  StemFn        preprocess: Conv2d(1,64,7,s2,p3)+BN+ReLU+MaxPool(3,2,1)   residuals.py:209-216
  StemConvFn    the hourglass stem: Convolution(7,1,C,s2), no pool         stackHourglass.py:130-134
  ResidualFn    BasicBlock / Bottleneck / Residual (+downsample): one      residuals.py:34-165, 256-271
                chain over the block's own conv1..conv3
  UpsampleAddFn Upsample(2, nearest) + MergeUp of an hourglass level       hourglass.py:113-114
  DeconvBNFn    ConvTranspose2d(k4,s2,p1,no bias)+BN+ReLU                 residuals.py:286-310
  ConvBNFn      Convolution (conv+BN+ReLU) / conv+BN                      convolutions.py:25-49
  DeformConvFn  DCN: offset conv, sampled columns, 1x1 GEMM [+BN [+ReLU]]  deformable/dcn_v2.py:146-191
  DeformConvV2Fn  dcn_v2_conv with offset and mask as inputs               deformable/dcn_v2.py:14-92
  HeadsFn       all CenterNet terminals fused: one 3x3 GEMM with N = sum of
                hidden widths (+bias+ReLU epilogue) and the per-head 1x1s  centerNetOffset.py:103-122

Parameter gradients are accumulated straight into ``param.grad`` (created on demand;
with FlatAdam/FlatDDP they are views of one flat buffer), so the Functions return None
for parameter inputs.  Activations between Functions are NHWC in the model's compute dtype.

Every library launch is an ``ops`` function; what the folded inference path (scdhip.infer) shares with training -- the
stem's and the heads' forward dispatch -- is ``ops.stem_fwd`` / ``ops.heads_fwd``.
"""
import os

import torch

from . import ops
from .flat import grads_ready


def _c(t):
    return t if t is None or t.is_contiguous() else t.contiguous()


# stem backward as one pass (ops.stem_backward_fused); SCD_STEM_FUSED_BWD=0: pool backward + fused-apply weight gradient
_STEM_FUSED_BWD = os.environ.get("SCD_STEM_FUSED_BWD", "1") != "0"


def _conv_ld(w):
    """dst strides of an OIHW conv weight (Co, Ci, kh, kw) for scd_wgrad_reduce: [co][ci][tap]."""
    T = w.shape[2] * w.shape[3]
    return (w.shape[1] * T, T, 1)


def _conv_stats(x, conv, bn, stride, pad, training, timer=None):
    """conv (no bias) -> raw y, with the BN statistics accumulated in the GEMM epilogue (training)."""
    C = conv.weight.shape[0]
    kh, kw = conv.weight.shape[2], conv.weight.shape[3]
    wp = ops.pack_weight(conv.weight, x.dtype, 0)
    stats = ops.bn_stats(bn, "fwd") if training else None
    t0 = ops.LaunchTimer.record(timer) if timer else None
    y = ops.conv_fwd(x, wp, C, kh, kw, stride, pad, stats=stats)
    if timer:
        ops.LaunchTimer.close(timer, t0)
    return y, stats


def _train_bn_conv(x, conv, bn, stride, pad, training, timer=None):
    """conv (no bias) -> raw y + BN statistics -> BNState.  timer: LaunchTimer name for the GEMM (bench.py)."""
    C = conv.weight.shape[0]
    y, stats = _conv_stats(x, conv, bn, stride, pad, training, timer)
    return y, ops.bn_finalize(bn, stats, C, y.numel() // C, training)


def _conv1_and_downsample(x, dconv, bnd, conv1, bn1, s1, pad1, sd):
    """A block's first conv and its downsample conv (both read only the block input; residuals.py:99-120,
    145-165), then both BN finalizes together: with SyncBN one all-reduce for the two layers."""
    C1, Cd = conv1.weight.shape[0], dconv.weight.shape[0]
    y1, s1st = _conv_stats(x, conv1, bn1, s1, pad1, True)
    yd, sdst = _conv_stats(x, dconv, bnd, sd, 0, True)
    st1, std = ops.bn_finalize_pair(bn1, s1st, C1, y1.numel() // C1, bnd, sdst, Cd, yd.numel() // Cd)
    return y1, st1, yd, std


def _dgrad_bn_relu_bwd(dy, wpack_t, C, Hc, Wc, kh, kw, stride, pad, bn, st, y):
    """Input gradient of a conv whose input is a BN+ReLU layer's output (bn, st, pre-BN y), then that layer's
    backward.  In bf16 the dgrad GEMM's epilogue accumulates the BN backward sums (scd_conv_gemm_bnbwd; shapes
    outside the ping-pong kernel run GEMM + reduce inside the same entry point), so the BN backward is only the
    finalize + apply."""
    if dy.dtype in ops.HALF and ops.BNFusion.enabled:
        stats = ops.bn_stats(bn, "bwdf")
        da = ops.conv_dgrad(dy, wpack_t, C, Hc, Wc, kh, kw, stride, pad, bn_bwd=(st, y, stats))
        return ops.bn_backward(bn, st, da, y, relu=True, stats=stats)
    da = ops.conv_dgrad(dy, wpack_t, C, Hc, Wc, kh, kw, stride, pad)
    return ops.bn_backward(bn, st, da, y, relu=True)


class StemFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, conv, bn, dtype):
        training = bn.training
        C = conv.weight.shape[0]
        stats = ops.bn_stats(bn, "fwd") if training else None
        wpk = ops.pack_weight(conv.weight, dtype, 0, ldp=64)
        geom = tuple(conv.weight.shape) + (conv.stride[0], conv.padding[0])
        y, cols, direct = ops.stem_fwd(x, wpk, geom, dtype, stats)
        st = ops.bn_finalize(bn, stats, C, y.numel() // C, training)
        out, am = ops.stem_pool_fwd(y, st)
        ctx.save_for_backward(cols, y, am)
        ctx.st, ctx.conv, ctx.bn, ctx.direct = st, conv, bn, direct
        ctx.wpk = wpk if direct else None
        return out

    @staticmethod
    def backward(ctx, dout):
        conv, bn, st = ctx.conv, ctx.bn, ctx.st
        cols, y, am = ctx.saved_tensors
        if ctx.direct and _STEM_FUSED_BWD:
            # pool / ReLU / BN / weight-gradient backward in one pass over the pooled gradient (dz stays on chip)
            ops.stem_backward_fused(bn, _c(dout), am, y, st, cols, ctx.wpk, ops.grad_of(conv.weight))
        elif ctx.direct:
            # pool/ReLU backward + BN reduction in one pass; the BN apply runs inside the weight gradient
            dz, coef = ops.stem_pool_bwd_bn(bn, _c(dout), am, y, st)
            ops.stem_conv_wgrad(dz, cols, ops.grad_of(conv.weight), ybn=y, coef=coef)
        else:
            dz = ops.stem_pool_bwd(_c(dout), am, y, st)
            dy = ops.bn_backward(bn, st, dz, y)
            T = conv.weight.shape[2] * conv.weight.shape[3]
            ops.conv_wgrad(dy, cols, 1, 1, 1, 0, ops.grad_of(conv.weight), (T, 1, 0), cvalid=T)
        grads_ready(conv, bn)
        return None, None, None, None, None


class StemConvFn(torch.autograd.Function):
    """The hourglass stem, Convolution(7, 1, C, stride=2) on the NCHW fp32 input (stackHourglass.py:130-134): StemFn
    without the max-pool.  Any width but the direct kernel's 64 runs as im2col + a 1x1 GEMM (ops.stem_fwd)."""

    @staticmethod
    def forward(ctx, x, w, conv, bn, dtype):
        training = bn.training
        C = conv.weight.shape[0]
        stats = ops.bn_stats(bn, "fwd") if training else None
        wpk = ops.pack_weight(conv.weight, dtype, 0, ldp=64)
        geom = tuple(conv.weight.shape) + (conv.stride[0], conv.padding[0])
        y, cols, direct = ops.stem_fwd(x, wpk, geom, dtype, stats)
        if direct:
            raise NotImplementedError("StemConvFn keeps the im2col columns for its weight gradient; the 64-channel "
                                      "direct stem belongs to StemFn")
        st = ops.bn_finalize(bn, stats, C, y.numel() // C, training)
        out = ops.bn_apply(y, st, True)
        ctx.save_for_backward(cols, y)
        ctx.st, ctx.conv, ctx.bn = st, conv, bn
        return out

    @staticmethod
    def backward(ctx, dout):
        conv, bn, st = ctx.conv, ctx.bn, ctx.st
        cols, y = ctx.saved_tensors
        dy = ops.bn_backward(bn, st, _c(dout), y, relu=True)
        T = conv.weight.shape[2] * conv.weight.shape[3]
        ops.conv_wgrad(dy, cols, 1, 1, 1, 0, ops.grad_of(conv.weight), (T, 1, 0), cvalid=T)
        grads_ready(conv, bn)
        return None, None, None, None, None


class UpsampleAddFn(torch.autograd.Function):
    """Upsample(scale_factor=2, nearest) + MergeUp of one hourglass level (hourglass.py:113-114): up + nearest_2x(low)
    in one pass; backward hands dout itself to `up` and its 2x2 block sums to `low`."""

    @staticmethod
    def forward(ctx, up, low):
        return ops.upsample_add(up, low)

    @staticmethod
    def backward(ctx, dout):
        dout = _c(dout)
        return dout, ops.upsample_add_bwd(dout)


def _block_layers(blk):
    """(conv, bn, weight, (kh, kw, stride, pad)) of a BasicBlock's / Bottleneck's main branch, in order (the walk of
    infer.FoldedBlock): the geometry is the Conv2d modules' own."""
    mods = [(blk.conv1, blk.bn1), (blk.conv2, blk.bn2)]
    if "conv3" in blk._modules:
        mods.append((blk.conv3, blk.bn3))
    return [(c, bn, c.weight, (c.kernel_size[0], c.kernel_size[1], c.stride[0], c.padding[0])) for c, bn in mods]


class ResidualFn(torch.autograd.Function):
    """BasicBlock (two convs) and Bottleneck (three): conv + BN + ReLU down the main branch, the last BN joined with
    the identity or with the 1x1 downsample conv's BN, then the ReLU."""

    @staticmethod
    def forward(ctx, x, w1, blk):
        tr = blk.training
        layers = _block_layers(blk)
        dconv, dbn = blk.downsample if blk.downsample is not None else (None, None)
        yd = std = None
        saved, sts, a = [], [], x               # saved: each conv's input and pre-BN output
        for i, (conv, bn, _, (_, _, s, p)) in enumerate(layers):
            if i == 0 and tr and dconv is not None:
                y, st, yd, std = _conv1_and_downsample(x, dconv, dbn, conv, bn, s, p, dconv.stride[0])
            else:
                y, st = _train_bn_conv(a, conv, bn, s, p, tr)
            saved += [a, y]
            sts.append(st)
            if i + 1 < len(layers):
                a = ops.bn_apply(y, st, True)
        if dconv is not None:
            if yd is None:                      # eval: the downsample conv after the main branch
                yd, std = _train_bn_conv(x, dconv, dbn, dconv.stride[0], 0, tr)
            out = ops.bn_apply(y, st, True, res=yd, rst=std)
        else:
            out = ops.bn_apply(y, st, True, res=x)
        ctx.save_for_backward(*saved, yd, out)
        ctx.sts = (sts, std)
        ctx.blk, ctx.layers, ctx.down = blk, layers, (dconv, dbn)
        return out

    @staticmethod
    def backward(ctx, dout):
        *saved, yd, out = ctx.saved_tensors
        sts, std = ctx.sts
        layers, (dconv, dbn) = ctx.layers, ctx.down
        ins, ys = saved[0::2], saved[1::2]      # conv i reads ins[i] (ins[0] is the block input) and writes ys[i]
        x = ins[0]
        _, H, W, Cin = x.shape
        dx = dyd = None

        def wgrad(i, dy, dst):
            ops.conv_wgrad(dy, ins[i], *layers[i][3], dst, _conv_ld(layers[i][2]))

        n = len(layers) - 1
        _, bnn, wn, _ = layers[n]
        if dconv is not None:
            dy, dyd = ops.bn_backward_pair(bnn, sts[n], ys[n], dbn, std, yd, _c(dout), out)
            wd = dconv.weight
            gd, gn = ops.grad_of(wd), ops.grad_of(wn)      # (before the ordering: may zero-fill on this stream)
            with ops.side_batch():          # both weight gradients behind one side-stream ordering
                ops.conv_wgrad(dyd, x, 1, 1, dconv.stride[0], 0, gd, _conv_ld(wd))
                wgrad(n, dy, gn)
        else:
            dx = torch.empty_like(x)
            dy = ops.bn_backward(bnn, sts[n], _c(dout), ys[n], mask=out, dz_out=dx)
            wgrad(n, dy, ops.grad_of(wn))
        for i in range(n, 0, -1):
            _, _, w, geom = layers[i]
            dy = _dgrad_bn_relu_bwd(dy, ops.pack_weight(w, x.dtype, 1), w.shape[1], ins[i].shape[1], ins[i].shape[2],
                                    *geom, layers[i - 1][1], sts[i - 1], ys[i - 1])
            wgrad(i - 1, dy, ops.grad_of(layers[i - 1][2]))
        _, _, w1, (_, _, s1, p1) = layers[0]
        dx = ops.conv_dgrad_w(dy, w1, H, W, s1, p1, out=dx, accumulate=dx is not None)
        if dyd is not None:
            # the downsample's input gradient last: += over the pixels its 1x1 taps reach only (one in four at stride 2)
            ops.conv_dgrad(dyd, ops.pack_weight(wd, x.dtype, 1), Cin, H, W, 1, 1, dconv.stride[0], 0, out=dx,
                           accumulate=True)
        grads_ready(ctx.blk)
        return dx, None, None


class DeconvBNFn(torch.autograd.Function):
    """ConvTranspose2d(k, s=2, p, op=0, bias=False) -> BN -> ReLU.  The deconv forward is the
    input-gradient of the Conv2d whose weight is W_t (4 sub-pixel phases of 2x2 taps each)."""

    @staticmethod
    def forward(ctx, x, w, deconv, bn):
        k = w.shape[2]
        s, p = deconv.stride[0], deconv.padding[0]
        Cout = w.shape[1]
        stats = ops.bn_stats(bn, "fwd") if bn.training else None
        y = ops.deconv_fwd(x, ops.pack_weight(w, x.dtype, 1), Cout, k, s, p, stats=stats)
        st = ops.bn_finalize(bn, stats, Cout, y.numel() // Cout, bn.training)
        out = ops.bn_apply(y, st, True)
        ctx.save_for_backward(x, y, out)
        ctx.st, ctx.deconv, ctx.bn = st, deconv, bn
        ctx.prod = ops.bn_producer(x)           # a BN+ReLU layer before this one: its sums come from our dgrad
        ops.set_bn_producer(out, bn, st, y)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, y, out = ctx.saved_tensors
        deconv, bn, st = ctx.deconv, ctx.bn, ctx.st
        w = deconv.weight
        k = w.shape[2]
        s, p = deconv.stride[0], deconv.padding[0]
        dout = _c(dout)
        dy = ops.bn_backward(bn, st, dout, y, relu=True, stats=ops.take_bn_bwd_fused(bn, dout))
        # dW_t[i][o][r][s] = sum x[i at q] * dy[o at s*q + r - p]: weight-gradient GEMM with G = x
        T = k * k
        ops.conv_wgrad(x, dy, k, k, s, p, ops.grad_of(w), (w.shape[1] * T, T, 1))
        fuse = ctx.prod is not None and x.dtype in ops.HALF
        dx = ops.deconv_dgrad(dy, ops.pack_weight(w, x.dtype, 0), w.shape[0], k, s, p,
                              bn_bwd=ops.fused_bn_bwd_args(ctx.prod) if fuse else None)
        if fuse:
            ops.mark_bn_bwd_fused(ctx.prod[0], dx)
        grads_ready(deconv, bn)
        return dx, None, None, None


class ConvBNFn(torch.autograd.Function):
    """Conv2d(no bias, 'same' padding) -> BN -> [ReLU] (Convolution, convolutions.py:25-49)."""

    @staticmethod
    def forward(ctx, x, w, conv, bn, relu):
        s, p = conv.stride[0], conv.padding[0]
        y, st = _train_bn_conv(x, conv, bn, s, p, bn.training)
        out = ops.bn_apply(y, st, relu)
        ctx.save_for_backward(x, y, out)
        ctx.st, ctx.conv, ctx.bn, ctx.relu = st, conv, bn, relu
        return out

    @staticmethod
    def backward(ctx, dout):
        x, y, out = ctx.saved_tensors
        conv, bn, st = ctx.conv, ctx.bn, ctx.st
        w = conv.weight
        kh, kw = w.shape[2], w.shape[3]
        s, p = conv.stride[0], conv.padding[0]
        dy = ops.bn_backward(bn, st, _c(dout), y, relu=ctx.relu)
        ops.conv_wgrad(dy, x, kh, kw, s, p, ops.grad_of(w), _conv_ld(w))
        dx = ops.conv_dgrad(dy, ops.pack_weight(w, x.dtype, 1), x.shape[3], x.shape[1], x.shape[2], kh, kw, s, p)
        grads_ready(conv, bn)
        return dx, None, None, None, None


def _dcn_conv_fwd(x, om, G, sigmoid, w, bias, stats=None):
    """The deformable conv proper: sampled columns (N,H,W,9C), then the 1x1 GEMM over them with w's pack mode 0."""
    cols = ops.dcn_cols(x, om, G, sigmoid)
    y = ops.conv_fwd(cols, ops.pack_weight(w, x.dtype, 0), w.shape[0], 1, 1, 1, 0, bias=bias, stats=stats)
    return cols, y


def _dcn_cols_grad(dy, w):
    """Gradient towards the columns: a 1x1 GEMM with the transposed weight, rows tap-major (pack mode 2)."""
    return ops.conv_fwd(dy, ops.pack_concat([w], dy.dtype, 2), 9 * w.shape[1], 1, 1, 1, 0)


class DeformConvFn(torch.autograd.Function):
    """DCN (models/backbones/deformable/dcn_v2.py:146-191 of the reference): offsets and mask logits from the module's
    own conv_offset_mask, the modulated deformable 3x3 conv with bias, then optionally BatchNorm2d [+ ReLU]."""

    @staticmethod
    def forward(ctx, x, w, dcn, bn, relu):
        ops._need_gpu(x, w)
        G, com = dcn.deformable_groups, dcn.conv_offset_mask
        P = ops.dcn_om_channels(G, x.dtype)
        wo, bo = ops.dcn_offset_rows(com.weight, com.bias, P)
        om = ops.conv_fwd(x, ops.pack_weight(wo, x.dtype, 0), P, 3, 3, 1, 1, bias=bo)
        Co = dcn.weight.shape[0]
        training = bn is not None and bn.training
        stats = ops.bn_stats(bn, "fwd") if training else None
        cols, y = _dcn_conv_fwd(x, om, G, True, dcn.weight, dcn.bias, stats)
        if bn is None:
            out, st = y, None
        else:
            st = ops.bn_finalize(bn, stats, Co, y.numel() // Co, training)
            out = ops.bn_apply(y, st, relu)
        ctx.save_for_backward(x, om, cols, y)
        ctx.st, ctx.dcn, ctx.bn, ctx.relu = st, dcn, bn, relu
        return out

    @staticmethod
    def backward(ctx, dout):
        x, om, cols, y = ctx.saved_tensors
        dcn, bn, st = ctx.dcn, ctx.bn, ctx.st
        G, com, w = dcn.deformable_groups, dcn.conv_offset_mask, dcn.weight
        N, H, W, C = x.shape
        dy = _c(dout) if bn is None else ops.bn_backward(bn, st, _c(dout), y, relu=ctx.relu)
        alpha = ops.grad_alpha(dy)
        # the columns are the 1x1 GEMM's input: its 9C workspace columns are reduced as 9 taps x C into the OIHW rows
        ops.conv_wgrad(dy, cols, 1, 1, 1, 0, None, None, rows=[(0, w.shape[0], ops.grad_of(w), _conv_ld(w))],
                       red_taps=9)
        ops.grad_of(dcn.bias).add_(dy.sum((0, 1, 2), dtype=torch.float32), alpha=alpha)
        dx32, dom = ops.dcn_cols_bwd(_dcn_cols_grad(dy, w), x, om, G, True)
        dx = dx32.to(x.dtype)
        n_om = com.weight.shape[0]
        ops.conv_wgrad(dom, x, 3, 3, 1, 1, None, None,
                       rows=[(0, n_om, ops.grad_of(com.weight), _conv_ld(com.weight))])
        ops.grad_of(com.bias).add_(dom[..., :n_om].sum((0, 1, 2), dtype=torch.float32), alpha=alpha)
        wo, _ = ops.dcn_offset_rows(com.weight, com.bias, om.shape[3])
        ops.conv_dgrad(dom, ops.pack_weight(wo, x.dtype, 1), C, H, W, 3, 3, 1, 1, out=dx, accumulate=True)
        grads_ready(*([dcn] if bn is None else [dcn, bn]))
        return dx, None, None, None, None


class DeformConvV2Fn(torch.autograd.Function):
    """dcn_v2_conv (dcn_v2.py:14-92 of the reference) on NHWC tensors: offset (N,H,W,18G) and mask (N,H,W,9G) are
    inputs, every tensor input gets its gradient back."""

    @staticmethod
    def forward(ctx, x, offset, mask, weight, bias, G):
        ops._need_gpu(x, offset, mask, weight, bias)
        N, H, W, _ = x.shape
        P = ops.dcn_om_channels(G, x.dtype)
        om = torch.zeros(N, H, W, P, dtype=x.dtype, device=x.device)
        om[..., :18 * G] = offset
        om[..., 18 * G:27 * G] = mask
        cols, y = _dcn_conv_fwd(x, om, G, False, weight, bias)
        ctx.save_for_backward(x, om, cols, weight)
        ctx.G = G
        return y

    @staticmethod
    def backward(ctx, dout):
        x, om, cols, w = ctx.saved_tensors
        G = ctx.G
        dy = _c(dout)
        dw = torch.zeros_like(w)
        # on the current stream: autograd hands dw on as soon as this returns
        ops._conv_wgrad(dy, cols, 1, 1, 1, 0, None, None, rows=[(0, w.shape[0], dw, _conv_ld(w))], red_taps=9)
        db = dy.sum((0, 1, 2), dtype=torch.float32) * ops.grad_alpha(dy)
        dx32, dom = ops.dcn_cols_bwd(_dcn_cols_grad(dy, w), x, om, G, False)
        return (dx32.to(x.dtype), dom[..., :18 * G].contiguous(), dom[..., 18 * G:27 * G].contiguous(), dw, db, None)


class HeadsFn(torch.autograd.Function):
    """All CenterNet terminals (Conv2d 3x3 +bias -> ReLU -> Conv2d 1x1 +bias) fused:
    hidden = relu(conv3x3(feat, W0cat) + b0cat) with N = sum of hidden widths, then the
    block-diagonal 1x1 tails.  Outputs are NCHW fp32, one tensor per head."""

    @staticmethod
    def forward(ctx, feat, w0_first, heads):
        N, H, W, Cin = feat.shape
        w0s = [h[0].weight for h in heads]
        b0 = torch.cat([h[0].bias for h in heads], 0)
        hd = ops.HeadsDesc([h[2].weight for h in heads], [h[2].bias for h in heads])
        wp = ops.pack_concat(w0s, feat.dtype, 0)
        hint = ops.take_sparse_hint()
        keep = ctx.keep = ctx.refill = None
        if (hd.fused and hint is not None and hd.nh >= 2 and Cin <= 256 and (hd.nh - 1) * hd.Hd <= 256
                and hint.dim() == 2 and hint.shape[0] == N):
            # the loss gathers the size / offset outputs at `hint` only: their hidden channels are stored there
            keep = ops.heads_keep_map(hint, N, H * W)
            ctx.keep = (hint, hint._version)
            ctx.refill = (wp, b0)       # what storing the whole hidden tensor again needs (a dense backward after all)
        hid, outs = ops.heads_fwd(feat, wp, b0, hd, keep)
        ctx.save_for_backward(feat, hid)
        ctx.w0s = w0s
        ctx.heads, ctx.hd = heads, hd
        ctx.prod = ops.bn_producer(feat)        # the deconv BN+ReLU: its backward sums come from our dgrad
        return tuple(outs)

    @staticmethod
    def backward(ctx, *douts):
        feat, hid = ctx.saved_tensors
        w0s = ctx.w0s
        heads, hd = ctx.heads, ctx.hd
        Hd, nh = hd.Hd, hd.nh
        N, H, W, Cin = feat.shape
        douts = [(_c(d) if d is not None else torch.zeros(N, o, H, W, device=feat.device))
                 for d, o in zip(douts, hd.od)]
        # fp16: the backward below runs on loss-scaled gradients (ops.LossScale: the repack multiplies the head
        # gradients by S), unscaled into every .grad
        S = ops.begin_loss_scale(feat.dtype)
        dptrs = ops.tensor_ptrs(douts)
        nd = HeadsFn._dense_prefix(douts, Hd, Cin)
        if ctx.keep is not None:
            inds = ops.sparse_grad_inds(douts[-1]) if nd == 1 else None
            if inds is None or inds is not ctx.keep[0] or inds._version != ctx.keep[1]:
                # the forward kept the size / offset hidden channels at other pixels only: store them all
                ops.heads_refill(feat, *ctx.refill, hd, hid)
            ctx.refill = None
        if nd < nh:
            return HeadsFn._backward_sparse(ctx, douts, dptrs, hd.odarr, nd, S)
        dhid = ops.heads_bwd_packed(hid, hd, dptrs, S)
        ops.heads_bwd_weight_finalize(hd, [h[0].bias for h in heads], S)
        ld = (Cin * 9, 9, 1)
        rows = [(i * Hd, (i + 1) * Hd, ops.grad_of(h[0].weight), ld) for i, h in enumerate(heads)]
        ops.conv_wgrad(dhid, feat, 3, 3, 1, 1, None, None, rows=rows)
        # feat's gradient shared with other consumers (ops.share_grad): write into / start the one buffer, and no
        # BN-backward sums from this epilogue (they would cover this consumer's part only)
        slot = ops.shared_grad_slot(feat)
        prev = slot[1] if slot is not None else None
        fuse = slot is None and ctx.prod is not None and feat.dtype in ops.HALF
        dfeat = ops.conv_dgrad(dhid, ops.pack_concat(w0s, feat.dtype, 1), Cin, H, W, 3, 3, 1, 1, out=prev,
                               accumulate=prev is not None, bn_bwd=ops.fused_bn_bwd_args(ctx.prod) if fuse else None)
        if fuse:
            ops.mark_bn_bwd_fused(ctx.prod[0], dfeat)
        grads_ready(*[m for h in heads for m in h if isinstance(m, torch.nn.Module)])
        if slot is not None:
            return ops.shared_grad_out(feat, slot, dfeat if prev is None else None), None, None
        return dfeat, None, None

    @staticmethod
    def _dense_prefix(douts, Hd, Cin):
        """Number of leading heads that need the dense backward: the rest must carry the loss's sparse-support
        certificate (one index tensor for all of them; ops.certify_sparse_grad)."""
        nh = len(douts)
        if nh < 2 or Cin > 256:
            return nh
        certs = [ops.sparse_grad_inds(d) for d in douts]
        nd = nh
        while nd > 1 and certs[nd - 1] is not None and certs[nd - 1] is certs[-1]:
            nd -= 1
        return nd if (nh - nd) * Hd <= 256 else nh

    @staticmethod
    def _backward_sparse(ctx, douts, dptrs, odarr, nd, S):
        """Heads [0, nd): the dense tail backward and 3x3 GEMMs over their nd*Hd hidden channels.  Heads [nd, nh):
        their output gradient lives on the certified pixels inds[b][k] only, so the tail backward, the 3x3 weight
        gradient (a GEMM over those pixels' im2col rows) and the 3x3 input gradient (a small GEMM then a gather
        into the dense input gradient) run over that pixel set (scd_heads_sparse_bwd / scd_heads_sparse_fixup)."""
        feat, hid = ctx.saved_tensors
        w0s, heads, hd = ctx.w0s, ctx.heads, ctx.hd
        Hd, nh = hd.Hd, hd.nh
        N, H, W, Cin = feat.shape
        dt = feat.dtype
        inds = ops.sparse_grad_inds(douts[-1])
        Sl = N * inds.shape[1]                         # slots
        Cs = (nh - nd) * Hd
        dh_dense = ops.heads_bwd_packed(hid, hd, dptrs, S, nd)
        dhid_s, xcol, slotmap, ownermap = ops.heads_sparse_bwd(hid, feat, hd, nd, dptrs, S, inds)
        ops.heads_bwd_weight_finalize(hd, [h[0].bias for h in heads], S)
        # weight gradients: dense heads over every pixel, sparse heads over the slots' im2col rows (a 1x1 GEMM whose
        # Cin*9 columns are the OIHW rows of their 3x3 weights)
        ld = (Cin * 9, 9, 1)

        def wgrads():
            # (the gradient views first -- they may zero-fill on this stream -- then both GEMMs behind one
            # side-stream ordering)
            rd = [(i * Hd, (i + 1) * Hd, ops.grad_of(heads[i][0].weight), ld) for i in range(nd)]
            rs = [((i - nd) * Hd, (i - nd + 1) * Hd, ops.grad_of(heads[i][0].weight), ld) for i in range(nd, nh)]
            with ops.side_batch():
                ops.conv_wgrad(dh_dense, feat, 3, 3, 1, 1, None, None, rows=rd)
                # (a 1x1 GEMM over the slots; its 9*Cin columns are reduced as 9 taps x Cin into the OIHW rows)
                ops.conv_wgrad(dhid_s.view(1, 1, Sl, Cs), xcol.view(1, 1, Sl, 9 * Cin), 1, 1, 1, 0, None, None,
                               rows=rs, red_taps=9)
        # input gradient: dense heads' GEMM (+ the deconv BN's backward sums), then the sparse heads' part
        fuse = ctx.prod is not None and dt in ops.HALF
        bn_args = ops.fused_bn_bwd_args(ctx.prod) if fuse else None
        dfeat = ops.conv_dgrad(dh_dense, ops.pack_concat(w0s[:nd], dt, 1), Cin, H, W, 3, 3, 1, 1, bn_bwd=bn_args)
        wt_s = ops.pack_concat(w0s[nd:], dt, 2)          # [tap][ci][c] rows: W0^T of the sparse heads, tap-major
        cols = ops.conv_fwd(dhid_s.view(1, 1, Sl, Cs), wt_s, 9 * Cin, 1, 1, 1, 0)
        ops.heads_sparse_fixup(dfeat, cols, inds, slotmap, ownermap, bn_args)
        mods = [m for h in heads for m in h if isinstance(m, torch.nn.Module)]
        if fuse:
            ops.mark_bn_bwd_fused(ctx.prod[0], dfeat)
        wgrads()                 # side stream ordered after the input gradient: it overlaps the deconv backward
        grads_ready(*mods)
        return dfeat, None, None


class CornerPoolFn(torch.autograd.Function):
    """CornerPool module (cornerNetCPool.py:83-122) on NHWC activations:
    a_i = relu(bn(conv3x3(x)))  (branch1/2, Convolution);  s = pool1(a1) + pool2(a2)
    r = relu(bn(conv3x3(s)) + bn(conv1x1(x)));  out = relu(bn(conv3x3(r)))  (lastConv)."""

    @staticmethod
    def forward(ctx, x, w_anchor, mod, dirs):
        tr = mod.branchMergeBn.training
        b1, b2, lc = mod.branch1, mod.branch2, mod.lastConv
        if tr:
            # both branch convs read x: their BN finalizes together (one SyncBN all-reduce for the two)
            y1, s1 = _conv_stats(x, b1.conv, b1.bn, 1, 1, tr)
            y2, s2 = _conv_stats(x, b2.conv, b2.bn, 1, 1, tr)
            C1, C2 = b1.conv.weight.shape[0], b2.conv.weight.shape[0]
            st1, st2 = ops.bn_finalize_pair(b1.bn, s1, C1, y1.numel() // C1, b2.bn, s2, C2, y2.numel() // C2)
        else:
            y1, st1 = _train_bn_conv(x, b1.conv, b1.bn, 1, 1, tr)
            y2, st2 = _train_bn_conv(x, b2.conv, b2.bn, 1, 1, tr)
        a1 = ops.bn_apply(y1, st1, True)
        a2 = ops.bn_apply(y2, st2, True)
        p1 = ops.cpool_fwd(a1, dirs[0])
        t0 = ops.LaunchTimer.record("cpool_fwd_add")
        s = ops.cpool_fwd(a2, dirs[1], addend=p1)
        ops.LaunchTimer.close("cpool_fwd_add", t0)
        del p1
        if tr:
            ym, sm = _conv_stats(s, mod.branchMerge, mod.branchMergeBn, 1, 1, tr)
            ysc, ss = _conv_stats(x, mod.shortcutConv, mod.shortcutBn, 1, 0, tr)
            Cm, Cs = mod.branchMerge.weight.shape[0], mod.shortcutConv.weight.shape[0]
            stm, sts = ops.bn_finalize_pair(mod.branchMergeBn, sm, Cm, ym.numel() // Cm, mod.shortcutBn, ss, Cs,
                                            ysc.numel() // Cs)
        else:
            ym, stm = _train_bn_conv(s, mod.branchMerge, mod.branchMergeBn, 1, 1, tr)
            ysc, sts = _train_bn_conv(x, mod.shortcutConv, mod.shortcutBn, 1, 0, tr)
        r = ops.bn_apply(ym, stm, True, res=ysc, rst=sts)
        yl, stl = _train_bn_conv(r, lc.conv, lc.bn, 1, 1, tr, timer="cpool_lastconv")
        out = ops.bn_apply(yl, stl, True)
        ctx.save_for_backward(x, y1, a1, y2, a2, s, ym, ysc, r, yl, out)
        ctx.sts = (st1, st2, stm, sts, stl)
        ctx.mod, ctx.dirs = mod, dirs
        return out

    @staticmethod
    def backward(ctx, dout):
        x, y1, a1, y2, a2, s, ym, ysc, r, yl, out = ctx.saved_tensors
        st1, st2, stm, sts, stl = ctx.sts
        mod, dirs = ctx.mod, ctx.dirs
        N, H, W, C = x.shape
        lc = mod.lastConv
        dyl = ops.bn_backward(lc.bn, stl, _c(dout), yl, relu=True)
        ops.conv_wgrad(dyl, r, 3, 3, 1, 1, ops.grad_of(lc.conv.weight), _conv_ld(lc.conv.weight))
        dr = ops.conv_dgrad(dyl, ops.pack_weight(lc.conv.weight, x.dtype, 1), C, H, W, 3, 3, 1, 1)
        dym, dys = ops.bn_backward_pair(mod.branchMergeBn, stm, ym, mod.shortcutBn, sts, ysc, dr, r)
        wsc = mod.shortcutConv.weight
        ops.conv_wgrad(dys, x, 1, 1, 1, 0, ops.grad_of(wsc), _conv_ld(wsc))
        slot = ops.shared_grad_slot(x)          # x's gradient shared with the other heads (ops.share_grad)
        prev = slot[1] if slot is not None else None
        dx = ops.conv_dgrad(dys, ops.pack_weight(wsc, x.dtype, 1), C, H, W, 1, 1, 1, 0, out=prev,
                            accumulate=prev is not None)
        wm = mod.branchMerge.weight
        ops.conv_wgrad(dym, s, 3, 3, 1, 1, ops.grad_of(wm), _conv_ld(wm))
        Cb = wm.shape[1]
        ds = ops.conv_dgrad(dym, ops.pack_weight(wm, x.dtype, 1), Cb, H, W, 3, 3, 1, 1)
        for (a, y, st, br), d in zip(((a1, y1, st1, mod.branch1), (a2, y2, st2, mod.branch2)), dirs):
            da = ops.cpool_bwd(a, ds, d)
            dy = ops.bn_backward(br.bn, st, da, y, relu=True)
            ops.conv_wgrad(dy, x, 3, 3, 1, 1, ops.grad_of(br.conv.weight), _conv_ld(br.conv.weight))
            ops.conv_dgrad(dy, ops.pack_weight(br.conv.weight, x.dtype, 1), C, H, W, 3, 3, 1, 1, out=dx,
                           accumulate=True)
        grads_ready(mod)
        if slot is not None:
            return ops.shared_grad_out(x, slot, dx if prev is None else None), None, None, None
        return dx, None, None, None


class CPoolFn(torch.autograd.Function):
    """Directional corner pool (TopPoolFunction etc., cornerPooling/__init__.py:8-58) on NHWC."""

    @staticmethod
    def forward(ctx, x, direction):
        ctx.save_for_backward(x)
        ctx.direction = direction
        return ops.cpool_fwd(x, direction)


    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        return ops.cpool_bwd(x, _c(dy), ctx.direction), None


class NCHWToNHWC(torch.autograd.Function):
    """Layout boundary for callers that hand NCHW activations to a block (tests, custom heads)."""

    @staticmethod
    def forward(ctx, x, dtype):
        ctx.dtype_in = x.dtype
        return x.permute(0, 2, 3, 1).to(dtype).contiguous()

    @staticmethod
    def backward(ctx, g):
        return g.permute(0, 3, 1, 2).to(ctx.dtype_in).contiguous(), None
