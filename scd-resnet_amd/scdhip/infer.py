"""Folded-BatchNorm inference of the CenterNet ResNet family.

BatchNorm on running statistics is a fixed per-channel affine map, so it belongs in the conv weights: ``fold(model)``
snapshots a model's parameters and buffers into packed operands w' = w * s and fp32 biases b' = beta - mean * s
(s = gamma / sqrt(var + eps)) and runs every block conv, downsample conv and deconv as one ``scd_conv_gemm_res`` launch
whose epilogue adds the bias and, at a block's join, the identity in fp32 before the ReLU and the one rounding at the
store.  The eval path of the training forward (a GEMM that writes the pre-BN output, ``scd_bn_finalize``, then
``scd_bn_apply`` reading it back) needs three passes per layer and repacks through the training step's PackPlan; a
steady-state folded forward makes no ``scd_bn_*`` and no ``scd_pack_*`` call, runs under ``no_grad`` and saves nothing.

The stem keeps its kernels (raw-weight stem conv, then ``scd_stem_pool_fwd``, which already fuses the BN scale / shift,
the ReLU and the pool) behind ``ops.stem_fwd``, the dispatch ``blocks.StemFn`` uses; the heads are ``ops.heads_fwd``, as
in ``blocks.HeadsFn.forward`` but without the training path's keep map, and the decode is the model's decoder.
"""
import torch

from . import ops


def fold_conv_bn(weight, bn, transposed=False, conv_bias=None):
    """(w', b') with conv(x, w') + b' == bn_eval(conv(x, weight) + conv_bias).  `bn` carries weight, bias,
    running_mean, running_var and eps (a BatchNorm2d); `transposed`: `weight` is a ConvTranspose2d weight (output
    channels along dim 1).  Computed in float64, returned in fp32; plain torch on the tensors' device."""
    w = weight.detach().double()
    s = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
    shape = [1] * w.dim()
    shape[1 if transposed else 0] = -1
    b = bn.bias.detach().double() - bn.running_mean.detach().double() * s
    if conv_bias is not None:
        b = b + s * conv_bias.detach().double()
    return (w * s.view(shape)).float().contiguous(), b.float().contiguous()


def _pack(w, dtype, mode, ldp=None):
    # a fold-time pack of a plain tensor: never through the training step's PackPlan
    return ops.pack_weight(w.detach().float().contiguous(), dtype, mode, ldp, _cache=False)


def _need_cuda(t, what):
    if not t.is_cuda:
        raise RuntimeError("scdhip.infer: %s is on the CPU; the folded operands are packed on the GPU (move the "
                           "model to the device first)" % what)


class _Conv:
    """One folded Conv2d + BatchNorm2d: packed operand in `dtype`, fp32 bias."""

    def __init__(self, conv, bn, dtype):
        _need_cuda(conv.weight, type(conv).__name__)
        if conv.bias is not None and bn is None:
            raise NotImplementedError("conv with bias and no BatchNorm")
        if conv.kernel_size[0] != conv.kernel_size[1] or conv.stride[0] != conv.stride[1] \
                or conv.padding[0] != conv.padding[1] or conv.dilation != (1, 1) or conv.groups != 1:
            raise NotImplementedError("conv geometry %r" % (conv,))
        w, b = fold_conv_bn(conv.weight, bn, conv_bias=conv.bias)
        self.Co, self.k, self.stride, self.pad = w.shape[0], w.shape[2], conv.stride[0], conv.padding[0]
        self.w, self.b = _pack(w, dtype, 0), b

    def __call__(self, x, relu, res=None):
        return ops.conv_fwd_res(x, self.w, self.Co, self.k, self.k, self.stride, self.pad, self.b, res, relu)


class FoldedBlock:
    """BasicBlock / Bottleneck: relu(conv_n(... relu(conv_1(x))) + identity), the join in the last GEMM's epilogue."""

    def __init__(self, blk, dtype):
        names = [n for n in ("conv1", "conv2", "conv3") if hasattr(blk, n)]
        self.convs = [_Conv(getattr(blk, n), getattr(blk, "bn" + n[-1]), dtype) for n in names]
        self.down = None
        if blk.downsample is not None:
            ds = blk.downsample
            if not (isinstance(ds, torch.nn.Sequential) and len(ds) == 2 and isinstance(ds[0], torch.nn.Conv2d)
                    and isinstance(ds[1], torch.nn.BatchNorm2d)):
                raise NotImplementedError("downsample branch %r" % (ds,))
            self.down = _Conv(ds[0], ds[1], dtype)
        self.dtype = dtype

    @torch.no_grad()
    def __call__(self, x):
        h = x
        for c in self.convs[:-1]:
            h = c(h, True)
        idn = x if self.down is None else self.down(x, False)
        return self.convs[-1](h, True, res=idn)


class FoldedDeconv:
    """ConvTranspose2d(k, s=2, p, no bias) + BatchNorm2d + ReLU as one four-phase GEMM with bias and ReLU."""

    def __init__(self, deconv, bn, dtype):
        _need_cuda(deconv.weight, "ConvTranspose2d")
        if deconv.bias is not None or deconv.output_padding != (0, 0):
            raise NotImplementedError("ConvTranspose2d with bias / output_padding")
        w, b = fold_conv_bn(deconv.weight, bn, transposed=True)
        self.Co, self.k, self.stride, self.pad = w.shape[1], w.shape[2], deconv.stride[0], deconv.padding[0]
        self.w, self.b = _pack(w, dtype, 1), b
        self.dtype = dtype

    @torch.no_grad()
    def __call__(self, x):
        return ops.deconv_fwd_res(x, self.w, self.Co, self.k, self.stride, self.pad, self.b, None, True)


class FoldedDeform:
    """DCN + BatchNorm2d + ReLU (a ResNet-DCN stage): the offset conv with its bias, the sampled columns
    (``scd_dcn_cols``), then one 1x1 GEMM over them with BN folded into the operand, plus bias and ReLU."""

    def __init__(self, dcn, bn, dtype):
        _need_cuda(dcn.weight, "DCN")
        com = dcn.conv_offset_mask
        self.G, self.Co = dcn.deformable_groups, dcn.weight.shape[0]
        self.P = ops.dcn_om_channels(self.G, dtype)
        wo, bo = ops.dcn_offset_rows(com.weight, com.bias, self.P)
        self.wo, self.bo = _pack(wo, dtype, 0), bo.detach().float().contiguous()
        w, b = fold_conv_bn(dcn.weight, bn, conv_bias=dcn.bias)
        self.w, self.b = _pack(w, dtype, 0), b
        self.dtype = dtype

    @torch.no_grad()
    def __call__(self, x):
        om = ops.conv_fwd_res(x, self.wo, self.P, 3, 3, 1, 1, self.bo, None, False)
        cols = ops.dcn_cols(x, om, self.G, True)
        return ops.conv_fwd_res(cols, self.w, self.Co, 1, 1, 1, 0, self.b, None, True)


def fold_block(blk, dtype):
    """A BasicBlock / Bottleneck as a callable NHWC -> NHWC that owns its folded operands (packed once in `dtype`)."""
    from models.backbones.residuals import BasicBlock, Bottleneck
    if not isinstance(blk, (BasicBlock, Bottleneck)):
        raise NotImplementedError("fold_block: %s" % type(blk).__name__)
    return FoldedBlock(blk, dtype)


def fold_deconv(deconv, bn, dtype):
    """ConvTranspose2d + BatchNorm2d + ReLU as a callable NHWC -> NHWC that owns its folded operand."""
    return FoldedDeconv(deconv, bn, dtype)


class _Stem:
    """Conv2d(1,64,7,s2,p3) + BN + ReLU + MaxPool(3,2,1): the training path's kernels on the raw weight, the eval
    scale / shift computed once."""

    def __init__(self, conv, bn, dtype):
        _need_cuda(conv.weight, "stem")
        self.dtype = dtype
        self.geom = tuple(conv.weight.shape) + (conv.stride[0], conv.padding[0])
        self.w = _pack(conv.weight, dtype, 0, ldp=64)
        s = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
        self.st = ops.BNState()
        self.st.scale = s.float().contiguous()
        self.st.shift = (bn.bias.detach().double() - bn.running_mean.detach().double() * s).float().contiguous()

    def __call__(self, x):
        y, _, _ = ops.stem_fwd(x.float().contiguous(), self.w, self.geom, self.dtype)
        return ops.stem_pool_fwd(y, self.st)[0]


class _Heads:
    """Plain CenterNet terminals of one hidden width: one 3x3 GEMM (+bias, ReLU) and the 1x1 tails."""

    def __init__(self, names, mods, dtype):
        self.names = names
        self.w0 = _pack(torch.cat([m[0].weight.detach() for m in mods], 0), dtype, 0)
        self.b0 = torch.cat([m[0].bias.detach().float() for m in mods], 0).contiguous()
        self.desc = ops.HeadsDesc([m[2].weight.detach().float().clone().contiguous() for m in mods],
                                  [m[2].bias.detach().float().clone().contiguous() for m in mods])

    def __call__(self, feat):
        return dict(zip(self.names, ops.heads_fwd(feat, self.w0, self.b0, self.desc)[1]))


class FoldedResNet(torch.nn.Module):
    """``fold(model)``: the model's eval-mode forward with BatchNorm folded into the conv operands.  A snapshot of
    the model's parameters and buffers at fold time in its ``compute_dtype``; ``refold()`` takes it again."""

    def __init__(self, model):
        super().__init__()
        self.__dict__["_source"] = model        # not a submodule: the folded net owns no parameters
        self.refold()

    @property
    def source(self):
        return self.__dict__["_source"]

    @torch.no_grad()
    def refold(self):
        from models.backbones.residuals import BasicBlock, Bottleneck, ResNet, _is_plain_head
        m = self.source
        if not isinstance(m, ResNet):
            raise NotImplementedError("fold: %s is not a scd ResNet" % type(m).__name__)
        dtype = m.compute_dtype
        # the heads first: a model this path does not cover is refused before anything is packed
        names = list(m.terminalLayers.keys())
        mods = [getattr(m, n) for n in names]
        for n, mod in zip(names, mods):
            if not _is_plain_head(mod):
                inner = mod[0] if isinstance(mod, torch.nn.Sequential) and len(mod) else mod
                raise NotImplementedError("fold: terminal '%s' (%s) is not a plain CenterNet head; the CornerPool "
                                          "model is not folded" % (n, type(inner).__name__))
        pre = m.preprocess
        if not (isinstance(pre, torch.nn.Sequential) and len(pre) == 4 and isinstance(pre[0], torch.nn.Conv2d)
                and isinstance(pre[1], torch.nn.BatchNorm2d) and isinstance(pre[3], torch.nn.MaxPool2d)
                and pre[0].in_channels == 1 and pre[0].stride == (2, 2) and pre[0].bias is None):
            raise NotImplementedError("fold: preprocess %s (only the default stem Conv7x7 s2 + BN + ReLU + MaxPool)"
                                      % type(pre).__name__)
        for layer in (m.layer1, m.layer2, m.layer3, m.layer4):
            for blk in layer:
                if not isinstance(blk, (BasicBlock, Bottleneck)):
                    raise NotImplementedError("fold: block %s" % type(blk).__name__)
        dl = m.deconvolutionLayers
        for i in range(0, len(dl), 3):
            if not isinstance(dl[i], torch.nn.ConvTranspose2d) or dl[i].bias is not None \
                    or dl[i].output_padding != (0, 0) or not isinstance(dl[i + 1], torch.nn.BatchNorm2d):
                raise NotImplementedError("fold: deconvolution layer %s (bias-free ConvTranspose2d + BatchNorm2d only)"
                                          % type(dl[i]).__name__)
        self.dtype = dtype
        self.stem = _Stem(pre[0], pre[1], dtype)
        self.blocks = [FoldedBlock(blk, dtype) for layer in (m.layer1, m.layer2, m.layer3, m.layer4) for blk in layer]
        self.deconvs = [FoldedDeconv(dl[i], dl[i + 1], dtype) for i in range(0, len(dl), 3)]
        # ResNet-DCN: the deformable stage in front of each deconv
        self.deforms = [FoldedDeform(d[0], d[1], dtype) for d in m.deformLayers] if getattr(m, "deformable", False) else None
        if len({mod[0].weight.shape[0] for mod in mods}) == 1:
            self.heads = [_Heads(names, mods, dtype)]
        else:
            self.heads = [_Heads([n], [mod], dtype) for n, mod in zip(names, mods)]
        self.names = names
        self.decoder = m.decoder
        return self

    @torch.no_grad()
    def forward(self, *x, **kwargs):
        inp = x[0]
        if not inp.is_cuda:
            raise RuntimeError("scd-resnet_amd executes on MI355X only (got a CPU input)")
        h = self.stem(inp)
        for blk in self.blocks:
            h = blk(h)
        for i, dc in enumerate(self.deconvs):
            if self.deforms is not None:
                h = self.deforms[i](h)
            h = dc(h)
        ret = {}
        for hd in self.heads:
            ret.update(hd(h))
        ret = {n: ret[n] for n in self.names}
        return [ret] if not kwargs.get("decode", False) else self.decoder(ret)


def fold(model):
    """The eval-mode forward of a CenterNet ResNet (default stem, BasicBlock / Bottleneck layers, bias-free deconvs,
    plain heads) with BatchNorm folded into the conv operands; anything else raises NotImplementedError."""
    return FoldedResNet(model)
