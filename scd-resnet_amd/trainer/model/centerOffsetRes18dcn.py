"""Model plugin `centerOffsetRes18dcn`: centerOffsetRes18 (same loss, dims, evaluation and expression) as a ResNet-DCN,
with a 3x3 modulated deformable conv + BN + ReLU (models/backbones/deformable) in front of each up-sampling stage.
Not in the reference, which ships the operator and wires it into no model.  Importing it reseeds torch with 42, as
every model plugin does."""
import torch

from models.centerNetOffset import CenterNetLoss, CenterNetResidual, centerNetEvaluation
from models.centerNetOffset import expression  # noqa: F401
from models.losses.focal import focalLoss
from models.losses.regression import L1LossMask

torch.random.manual_seed(42)

model = CenterNetResidual
loss = CenterNetLoss(0.1, 0.1, focal=focalLoss, regression=L1LossMask)
modelParams = {'numLayers': 18,
               'dims': [64, 64, 128, 256, 512, 256, 256, 256],
               'deformable': True}
evaluation = centerNetEvaluation
