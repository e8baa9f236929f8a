"""Pooling / unpooling layer builders (models/backbones/pooling.py of the reference).

The builders return the reference's torch modules.  On the HIP path the hourglass takes one combination of them:
no pooling layer (CenterNetHourglass down-samples with stride-2 Residuals) and ``unpoolingLayer(2)``, the nearest 2x
upsample that runs fused with the merge (blocks.UpsampleAddFn); Hourglass.forward refuses the others.
"""
from enum import Enum

import torch


class PoolingType(Enum):
    MaximalPool = 0
    AveragePool = 2


class UpsampleType(Enum):
    NearestNeighbour = 'nearest'
    Linear = 'linear'
    Bilinear = 'bilinear'
    Trilinear = 'trilinear'
    Bicubic = 'bicubic'


def poolingLayer(scaleFactor=2, downsampleType=PoolingType.MaximalPool, width=None, height=None):
    if downsampleType == PoolingType.MaximalPool:
        return torch.nn.MaxPool2d(kernel_size=scaleFactor, stride=scaleFactor)
    elif downsampleType == PoolingType.AveragePool:
        return torch.nn.AvgPool2d(kernel_size=scaleFactor, stride=scaleFactor)


def unpoolingLayer(scaleFactor=2, upsampleType=UpsampleType.NearestNeighbour):
    return torch.nn.Upsample(scale_factor=scaleFactor, mode=upsampleType.value)
