"""Stacked hourglass backbone + terminal wiring (models/backbones/stackHourglass.py of the reference) on libscdhip.

StackHourglass registers the reference's module tree in its order (preprocess, hourglassStack, redimConvolution, the
terminals, interHourglassLayers, shortcutLayers, convPrevHourglass, relu), so the state-dict keys are identical.  One
stack runs on HIP: with ``hourglassStacks == 1`` the three inter-stack lists are empty and no key is lost.

    preprocess[0]        Convolution(7, 1, C, stride=2) on the NCHW fp32 input    blocks.StemConvFn
    preprocess[1:]       Residual(3, C, dimensions[0], stride=2)                  blocks.ResidualFn
    hourglassStack[0]    models/backbones/hourglass.py                            ResidualFn, UpsampleAddFn
    redimConvolution[0]  Convolution(3, dimensions[0], predictionConvDim)         blocks.ConvBNFn
    terminals            Conv3x3 + bias + ReLU, Conv1x1, all of one hidden width  one blocks.HeadsFn

Activations between Functions are NHWC in the compute dtype; the terminal outputs are NCHW fp32, as the ResNet's.
"""
import torch

from models.backbones.convolutions import Convolution
from models.backbones.hourglass import Hourglass
from models.backbones.pooling import poolingLayer, unpoolingLayer
from models.backbones.residuals import Residual, residual3x3
from models.backbones.terminal import BackboneTerminal
from models.backbones.utility import changeDimensionConv, mergeLayer, stackLayers, stackLayersReverted
from scdhip import blocks, ops


class HourglassTerminal(BackboneTerminal):
    """Head descriptor (stackHourglass.py:49-61): name, output dims, initializer(module),
    makeLayer(predictionDim, currentDim, outputDim), process."""

    def __init__(self, name, outputDimension, initializerFunction=None, makeLayerFunction=None, process=None):
        super(HourglassTerminal, self).__init__(name, initializerFunction, makeLayerFunction, process)
        self.outputDimension = outputDimension


def _is_hourglass_head(m):
    """Sequential(Convolution(3, ., ., batchNorm=False), Conv2d 1x1): utility.convolutionConv1x1."""
    return (isinstance(m, torch.nn.Sequential) and len(m) == 2 and isinstance(m[0], Convolution)
            and not isinstance(m[0].bn, torch.nn.BatchNorm2d) and m[0].conv.kernel_size == (3, 3)
            and m[0].conv.stride == (1, 1) and m[0].conv.bias is not None and isinstance(m[1], torch.nn.Conv2d)
            and m[1].kernel_size == (1, 1) and m[1].bias is not None)


class StackHourglass(torch.nn.Module):
    """StackHourglass(hourglassIteration, hourglassStacks, dimensions, modules, outputDimension, ...) --
    stackHourglass.py:63-272.  ``compute_dtype`` as ResNet's (bf16 default)."""

    def __init__(self, hourglassIteration, hourglassStacks, dimensions, modules, outputDimension, beforeBackbone=None,
                 predictionConvDim=256, makeConvolutionLayer=changeDimensionConv, hourglassBeforeDownsample=stackLayers,
                 hourglassCentral=stackLayers, hourglassBefore=stackLayers, hourglassAfter=stackLayersReverted,
                 hourglassPool=poolingLayer, hourglassUnpooling=unpoolingLayer, hourglassMerge=mergeLayer,
                 makeInternalLayer=residual3x3, hourglassLayer=Residual, decoder=None, terminals=[]):
        super(StackHourglass, self).__init__()
        if hourglassStacks != 1:
            raise NotImplementedError("StackHourglass: %d stacks; one hourglass stack runs on HIP (the inter-stack "
                                      "shortcut layers are not built)" % hourglassStacks)
        self.hourglassStacks = hourglassStacks
        self.hourglassIteration = hourglassIteration
        self.decoder = decoder
        self.compute_dtype = torch.bfloat16
        cur = dimensions[0]
        self.preprocess = torch.nn.Sequential(
            Convolution(7, 3, 128, stride=2), Residual(3, 128, cur, stride=2)
        ) if beforeBackbone is None else beforeBackbone
        self.hourglassStack = torch.nn.ModuleList([
            Hourglass(hourglassIteration, dimensions, modules, layer=hourglassLayer,
                      layersBeforeDownsample=hourglassBeforeDownsample, layersCentral=hourglassCentral,
                      layersBeforeHourglass=hourglassBefore, layersAfterHourglass=hourglassAfter,
                      layersDownsampling=hourglassPool, layersUpsampling=hourglassUnpooling,
                      layersMerge=hourglassMerge) for _ in range(hourglassStacks)])
        self.redimConvolution = torch.nn.ModuleList([makeConvolutionLayer(cur, predictionConvDim)
                                                     for _ in range(hourglassStacks)])
        self.terminalLayers = {}
        self.terminals = {}
        for terminal in terminals:
            # (built on the host; the model is moved to the GPU as a whole)
            if terminal.makeLayer is not None:
                module = torch.nn.Sequential(*[terminal.makeLayer(predictionConvDim, cur, terminal.outputDimension)
                                               for _ in self.hourglassStack])
            else:
                module = torch.nn.Sequential(*[torch.nn.Sequential() for _ in self.hourglassStack])
            if terminal.initializer is not None:
                for layer in module:
                    terminal.initializer(layer)
            self.terminalLayers[terminal.name] = module
            self.terminals[terminal.name] = terminal
            setattr(self, terminal.name, module)
        self.interHourglassLayers = torch.nn.ModuleList([makeInternalLayer(cur) for _ in range(hourglassStacks - 1)])
        self.shortcutLayers = torch.nn.ModuleList([
            torch.nn.Sequential(torch.nn.Conv2d(cur, cur, (1, 1), bias=False), torch.nn.BatchNorm2d(cur))
            for _ in range(hourglassStacks - 1)])
        self.convPrevHourglass = torch.nn.ModuleList([
            torch.nn.Sequential(torch.nn.Conv2d(predictionConvDim, cur, (1, 1), bias=False), torch.nn.BatchNorm2d(cur))
            for _ in range(hourglassStacks - 1)])
        self.relu = torch.nn.ReLU(inplace=True)

    # ------------------------------------------------------------------ HIP execution
    def check_input(self, x):
        """Everything that can be refused before the first launch: the device, the stem's kind and the geometry (the
        reference fails at the merge's add when a level's map is odd)."""
        if not x.is_cuda:
            raise RuntimeError("scd-resnet_amd executes on MI355X only (got a CPU input); the CPU restatement "
                               "of the reference is oracle/ (test infrastructure)")
        pre = self.preprocess
        if not (isinstance(pre, torch.nn.Sequential) and len(pre) >= 1 and isinstance(pre[0], Convolution)
                and isinstance(pre[0].bn, torch.nn.BatchNorm2d) and pre[0].conv.in_channels == 1
                and pre[0].conv.stride == (2, 2) and all(isinstance(m, Residual) for m in pre[1:])):
            raise NotImplementedError("only a Convolution(k, 1, C, stride=2) + Residual stem runs on HIP")
        if x.dim() != 4 or x.shape[1] != 1:
            raise ValueError("StackHourglass: input %s, expected (N, 1, H, W)" % (tuple(x.shape),))
        H, W = x.shape[2], x.shape[3]
        step = 2 ** self.hourglassIteration
        if H % 4 or W % 4 or (H // 4) % step or (W // 4) % step:
            raise ValueError("StackHourglass: input %d x %d; the backbone works at H/4 x W/4, which its %d levels halve "
                             "%d times: H/4 and W/4 must be multiples of %d" % (H, W, self.hourglassIteration,
                                                                               self.hourglassIteration, step))

    def backbone_forward(self, x):
        """(N,1,H,W) fp32 NCHW (checked by forward) -> the prediction feature (N, H/4, W/4, predictionConvDim), NHWC
        compute dtype."""
        stem = self.preprocess[0]
        h = blocks.StemConvFn.apply(x.float().contiguous(), stem.conv.weight, stem.conv, stem.bn, self.compute_dtype)
        for m in self.preprocess[1:]:
            h = m(h)
        h = self.hourglassStack[0](h)
        return self.redimConvolution[0](h)

    def heads_forward(self, feat):
        names = list(self.terminalLayers.keys())
        mods = [getattr(self, n)[0] for n in names]
        for n, m in zip(names, mods):
            if not _is_hourglass_head(m):
                raise NotImplementedError("terminal '%s': only convolutionConv1x1 terminals (Conv3x3 + bias + ReLU, "
                                          "Conv1x1) run on HIP" % n)
        hm = [(m[0].conv, m[0].relu, m[1]) for m in mods]
        ret = {}
        if len({h[0].weight.shape[0] for h in hm}) == 1:
            # one fused call: feat has one consumer
            ret.update(zip(names, blocks.HeadsFn.apply(feat, hm[0][0].weight, hm)))
        else:
            ops.share_grad(feat, len(hm))
            for n, h in zip(names, hm):
                ret[n] = blocks.HeadsFn.apply(feat, h[0].weight, [h])[0]
        return ret

    def forward(self, *x, **kwargs):
        decode = kwargs.get("decode", False)
        self.check_input(x[0])
        # all packed weight operands of this step in one launch (scdhip.ops.PackPlan)
        plan = self.__dict__.get("_scd_packplan")
        if plan is None:
            plan = self.__dict__["_scd_packplan"] = ops.PackPlan()
        ops.pack_begin(plan)
        ret = self.heads_forward(self.backbone_forward(x[0]))
        return [ret] if not decode else self.decoder(ret)

    def set_compute_dtype(self, dtype):
        if dtype not in (torch.float32, torch.bfloat16, torch.float16):
            raise ValueError("compute dtype must be torch.float32, torch.bfloat16 or torch.float16")
        self.compute_dtype = dtype
        return self
