"""Modulated deformable convolution, DCNv2 (models/backbones/deformable/dcn_v2.py of the reference).

``DCNv2`` (:95-143), ``DCN`` (:146-191) and ``dcn_v2_conv`` (:92) keep the reference's names, constructor signatures,
parameter names, shapes and initialisation, so state dicts interchange key for key.  The compute runs on libscdhip
(scd_dcn_cols / scd_dcn_cols_bwd around the gather-GEMM; scdhip.blocks.DeformConvFn / DeformConvV2Fn) on NHWC
activations in the compute dtype, like every module here: ``input`` is (N,H,W,C), ``offset`` (N,H,W,18G), ``mask``
(N,H,W,9G), with offset channel 18g + 2k the row offset of tap k = 3i + j of deformable group g and 18g + 2k + 1 its
column offset.

Only what the ResNet-DCN family uses runs: a 3x3 kernel, stride 1, padding 1, dilation 1; any other geometry raises
NotImplementedError at construction.  Not built: the deformable PS-RoI pooling (``DCNv2Pooling`` / ``DCNPooling``,
:194-399) and the ONNX symbolic (:67-89, dcn_v2_onnx.py).
"""
import math

import torch
from torch.nn.modules.utils import _pair

from scdhip import blocks


def _check_geometry(kernel_size, stride, padding, dilation):
    if _pair(kernel_size) != (3, 3) or _pair(stride) != (1, 1) or _pair(padding) != (1, 1) \
            or _pair(dilation) != (1, 1):
        raise NotImplementedError("deformable conv: kernel %r stride %r padding %r dilation %r (the HIP kernels run "
                                  "kernel 3, stride 1, padding 1, dilation 1)"
                                  % (kernel_size, stride, padding, dilation))


def dcn_v2_conv(input, offset, mask, weight, bias, stride, padding, dilation, deformable_groups):
    """y = bias + sum over taps and channels of weight * mask * bilinear(input, tap position + offset), NHWC."""
    _check_geometry(tuple(weight.shape[2:4]), stride, padding, dilation)
    G = int(deformable_groups)
    if input.dim() != 4 or offset.shape != input.shape[:3] + (18 * G,) or mask.shape != input.shape[:3] + (9 * G,):
        raise ValueError("dcn_v2_conv: input %s needs offset (N,H,W,%d) and mask (N,H,W,%d), got %s and %s"
                         % (tuple(input.shape), 18 * G, 9 * G, tuple(offset.shape), tuple(mask.shape)))
    if weight.shape[1] != input.shape[3] or bias is None or bias.shape != (weight.shape[0],):
        raise ValueError("dcn_v2_conv: weight %s / bias do not fit %d input channels"
                         % (tuple(weight.shape), input.shape[3]))
    if not input.is_cuda:
        raise RuntimeError("scd-resnet_amd runs on MI355X only: got a CPU tensor (no CPU fallback; the CPU "
                           "restatement of the deformable conv is test infrastructure)")
    return blocks.DeformConvV2Fn.apply(input.contiguous(), offset.to(input.dtype), mask.to(input.dtype), weight, bias,
                                       G)


class DCNv2(torch.nn.Module):
    def __init__(self, in_channels, out_channels, kernel_size, stride, padding, dilation=1, deformable_groups=1):
        super(DCNv2, self).__init__()
        _check_geometry(kernel_size, stride, padding, dilation)
        if deformable_groups < 1 or in_channels % deformable_groups:
            raise ValueError("%d input channels in %d deformable groups" % (in_channels, deformable_groups))
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.kernel_size = _pair(kernel_size)
        self.stride = _pair(stride)
        self.padding = _pair(padding)
        self.dilation = _pair(dilation)
        self.deformable_groups = deformable_groups
        self.weight = torch.nn.Parameter(torch.empty(out_channels, in_channels, *self.kernel_size))
        self.bias = torch.nn.Parameter(torch.empty(out_channels))
        self.reset_parameters()

    def reset_parameters(self):
        bound = 1.0 / math.sqrt(self.in_channels * self.kernel_size[0] * self.kernel_size[1])
        torch.nn.init.uniform_(self.weight, -bound, bound)
        torch.nn.init.zeros_(self.bias)

    def forward(self, input, offset, mask):
        return dcn_v2_conv(input, offset, mask, self.weight, self.bias, self.stride, self.padding, self.dilation,
                           self.deformable_groups)


class DCN(DCNv2):
    """DCNv2 that draws offsets and masks from its own zero-initialised ``conv_offset_mask`` (27G channels: offsets in
    [0, 18G), mask logits in [18G, 27G)), so it starts as a plain 3x3 conv at half weight."""

    def __init__(self, in_channels, out_channels, kernel_size, stride, padding, dilation=1, deformable_groups=1):
        super(DCN, self).__init__(in_channels, out_channels, kernel_size, stride, padding, dilation,
                                  deformable_groups)
        self.conv_offset_mask = torch.nn.Conv2d(self.in_channels, 27 * self.deformable_groups,
                                                kernel_size=self.kernel_size, stride=self.stride,
                                                padding=self.padding, bias=True)
        self.init_offset()

    def init_offset(self):
        torch.nn.init.zeros_(self.conv_offset_mask.weight)
        torch.nn.init.zeros_(self.conv_offset_mask.bias)

    def forward(self, input):
        """input: NHWC activation (compute dtype) -> NHWC activation."""
        return blocks.DeformConvFn.apply(input.contiguous(), self.weight, self, None, False)
