"""One hourglass (models/backbones/hourglass.py of the reference), executed on libscdhip.

The module tree -- constructor signature, attribute names, registration order -- is the reference's, so the
state-dict keys are too.  The forward takes and returns NHWC activations in the compute dtype and runs

    up1  = preserveCurrentDimension(x)              Residual stack                       (blocks.ResidualFn)
    low1 = changeDimension(downSampling(x))         stride-2 Residual first, no pool     (blocks.ResidualFn)
    low2 = embeddedHourglass(low1)                  the next level, or the central stack
    low3 = changeDimensionBack(low2)                Residual stack
    out  = merge(up1, upSampling(low3))             one pass                             (blocks.UpsampleAddFn)

x feeds two Functions (up1 and the low path); autograd sums their two input gradients.
"""
import torch

from models.backbones.pooling import poolingLayer, unpoolingLayer
from models.backbones.residuals import Residual
from models.backbones.utility import MergeUp, mergeLayer, stackLayers, stackLayersReverted


class Hourglass(torch.nn.Module):
    """Hourglass(iterations, dimensions, modules, layer, layers*...) -- hourglass.py:31-114.  dimensions / modules hold
    iterations + 1 entries: level i works at dimensions[i] with modules[i] blocks per stack, the last entry is the
    centre."""

    def __init__(self, iterations, dimensions, modules, layer=Residual, layersBeforeDownsample=stackLayers,
                 layersCentral=stackLayers, layersBeforeHourglass=stackLayers, layersAfterHourglass=stackLayersReverted,
                 layersDownsampling=poolingLayer, layersUpsampling=unpoolingLayer, layersMerge=mergeLayer, **kwargs):
        super(Hourglass, self).__init__()
        self.iteration = iterations
        cur, nxt = dimensions[0], dimensions[1]
        self.preserveCurrentDimension = layersBeforeDownsample(3, cur, cur, modules[0], layer=layer, **kwargs)
        self.downSampling = layersDownsampling(2)
        self.changeDimension = layersBeforeHourglass(3, cur, nxt, modules[0], layer=layer, **kwargs)
        if iterations > 1:
            self.embeddedHourglass = Hourglass(
                iterations - 1, dimensions[1:], modules[1:], layer=layer, layersBeforeDownsample=layersBeforeDownsample,
                layersCentral=layersCentral, layersBeforeHourglass=layersBeforeHourglass,
                layersAfterHourglass=layersAfterHourglass, layersDownsampling=layersDownsampling,
                layersUpsampling=layersUpsampling, layersMerge=layersMerge, **kwargs)
        else:
            self.embeddedHourglass = layersCentral(3, nxt, nxt, modules[1], layer=layer, **kwargs)
        self.changeDimensionBack = layersAfterHourglass(3, nxt, cur, modules[0], layer=layer, **kwargs)
        self.upSampling = layersUpsampling(2)
        self.merge = layersMerge(cur)

    def check_layers(self):
        """The layer kinds the HIP path runs; anything else is refused before a launch."""
        ds, us = self.downSampling, self.upSampling
        if not (isinstance(ds, torch.nn.Sequential) and len(ds) == 0):
            raise NotImplementedError("Hourglass: down-sampling layer %s is not on the HIP path (CenterNetHourglass has "
                                      "none: its changeDimension stack starts with a stride-2 Residual)"
                                      % type(ds).__name__)
        if not (isinstance(us, torch.nn.Upsample) and us.mode == "nearest" and us.size is None
                and us.scale_factor in (2, 2.0, (2, 2), (2.0, 2.0))):
            raise NotImplementedError("Hourglass: only Upsample(scale_factor=2, mode='nearest') runs on the HIP path, "
                                      "got %r" % (us,))
        if not isinstance(self.merge, MergeUp):
            raise NotImplementedError("Hourglass: merge layer %s is not on the HIP path (MergeUp only)"
                                      % type(self.merge).__name__)

    def forward(self, x):
        self.check_layers()
        up1 = self.preserveCurrentDimension(x)
        low1 = self.changeDimension(x)
        low2 = self.embeddedHourglass(low1)
        low3 = self.changeDimensionBack(low2)
        return self.merge(up1, low3)
