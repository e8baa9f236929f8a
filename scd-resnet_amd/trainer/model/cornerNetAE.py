"""Model plugin `cornerNetAE`: CornerNetAEResidual(10), the corner-pooling CornerNet with embedding-tag heads that
outputs boxes (models/cornerNetAE.py).  It trains on a dataset plugin that serves the embedding layout
ys = [heat, mask, regr, tl, br, tl_inds, br_inds, valid]: `syntheticCorner` or a `.d` plugin `scdx{N}p{M}`, with the
configuration keys "cornerTargets": true and "cornerEmbeddings": true."""
import torch

from models.cornerNetAE import CornerNetAELoss, CornerNetAEResidual, cornerNetAEEvaluation, expression  # noqa: F401
from models.losses.focal import focalLoss

torch.random.manual_seed(42)

model = CornerNetAEResidual
loss = CornerNetAELoss(focal=focalLoss)
modelParams = {'numLayers': 10}
evaluation = cornerNetAEEvaluation
