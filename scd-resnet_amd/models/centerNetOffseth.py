"""CenterNet with 64-channel heads (models/centerNetOffseth.py of the reference: identical to
centerNetOffset.py except the terminal hidden width, :146-148), and the reference's other backbone for it, the
stacked hourglass (CenterNetHourglass, :52-101)."""
import torch

from models.backbones.convolutions import Convolution
from models.backbones.residuals import Residual
from models.backbones.stackHourglass import HourglassTerminal, StackHourglass
from models.backbones.utility import convolutionConv1x1
from models.centerNetOffset import (CLASSDIMENSION, CenterNetLoss, centerNetEvaluation, decodeCenterNet,  # noqa: F401
                                    expression, make_terminals, process)
from models.centerNetOffset import CenterNetResidual as _CenterNetResidual

resnetHeatmapTerminal, resnetSizeTerminal, resnetOffsetTerminal = make_terminals(64)


class CenterNetResidual(_CenterNetResidual):
    HEAD_DIM = 64


# ---- the hourglass terminals (:52-68): Conv3x3 + bias + ReLU -> Conv1x1, hidden width = the backbone's dimensions[0]

def heatmapInitializerHg(layer):
    layer[-1].bias.data.fill_(-2.19)


heatmapTerminalHg = HourglassTerminal("heatmap", CLASSDIMENSION, heatmapInitializerHg, convolutionConv1x1, process)
sizeRegressionTerminalHg = HourglassTerminal("regr", 4, None, convolutionConv1x1, process)
offsetRegressionTerminalHg = HourglassTerminal("offset", 2, None, convolutionConv1x1, process)


def makePoolLayer(dim):
    """No pooling layer (:70-71): the hourglass down-samples in makeHourglassLayer."""
    return torch.nn.Sequential()


def makeHourglassLayer(kernelSize, inputDimension, outputDimension, modules, layer=Convolution, **kwargs):
    """The stack in front of the embedded hourglass (:73-76): its first layer carries the stride 2."""
    layers = [layer(kernelSize, inputDimension, outputDimension, stride=2)]
    layers += [layer(kernelSize, outputDimension, outputDimension) for _ in range(modules - 1)]
    return torch.nn.Sequential(*layers)


class CenterNetHourglass(StackHourglass):
    """CenterNetHourglass() -- centerNetOffseth.py:78-101: five levels, one stack, 128-wide terminals on a 256-wide
    prediction feature.  The reference's constants are the defaults; ``hourglassIters``, ``dimensions``, ``modules``
    and ``predictionConvDim`` may be given by keyword (tests build a two-level net)."""

    def __init__(self, hourglassIters=5, dimensions=(128, 128, 192, 192, 192, 256), modules=(2, 2, 2, 2, 2, 4),
                 predictionConvDim=256, **kwargs):
        if kwargs:
            raise TypeError("CenterNetHourglass: unexpected arguments %s" % sorted(kwargs))
        dimensions, modules = list(dimensions), list(modules)
        if len(dimensions) != hourglassIters + 1 or len(modules) != hourglassIters + 1:
            raise ValueError("CenterNetHourglass: %d levels need %d dimensions and modules (got %d, %d)"
                             % (hourglassIters, hourglassIters + 1, len(dimensions), len(modules)))
        super(CenterNetHourglass, self).__init__(
            hourglassIters, 1, dimensions, modules, CLASSDIMENSION,
            hourglassPool=makePoolLayer, hourglassBefore=makeHourglassLayer, hourglassLayer=Residual,
            predictionConvDim=predictionConvDim,
            beforeBackbone=torch.nn.Sequential(Convolution(7, 1, 128, stride=2),
                                               Residual(3, 128, dimensions[0], stride=2)),
            terminals=[heatmapTerminalHg, sizeRegressionTerminalHg, offsetRegressionTerminalHg],
            decoder=decodeCenterNet)
