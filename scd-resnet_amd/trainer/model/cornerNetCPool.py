"""Model plugin `cornerNetCPool`: CornerNetResidual(10) with corner pooling (models/cornerNetCPool.py
of the reference; it ships no trainer/model plugin for it, this one follows the
centerOffsetRes10 layout).  It trains on any dataset plugin that serves the corner layout ys = [heat, mask, regr, tl, br]:
`syntheticCorner`, or a `.d` plugin `scdx{N}p{M}` with the configuration key "cornerTargets": true."""
import torch

from models.cornerNetCPool import CornerNetLoss, CornerNetResidual, cornerNetEvaluation, expression  # noqa: F401
from models.losses.focal import focalLoss

torch.random.manual_seed(42)

model = CornerNetResidual
loss = CornerNetLoss(focal=focalLoss)
modelParams = {'numLayers': 10}
evaluation = cornerNetEvaluation

