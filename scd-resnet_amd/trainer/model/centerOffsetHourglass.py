"""Model plugin `centerOffsetHourglass`: CenterNet on the reference's other backbone, the stacked hourglass (the
`# model = CenterNetHourglass` line of trainer/model/centerOffsetRes10.py:9-10 and its siblings).  Loss, evaluation
and expression are those of centerOffsetRes10; importing it reseeds torch with 42 like the other plugins."""
import torch

from models.centerNetOffset import CenterNetLoss, centerNetEvaluation
from models.centerNetOffset import expression  # noqa: F401
from models.centerNetOffseth import CenterNetHourglass
from models.losses.focal import focalLoss
from models.losses.regression import L1LossMask

torch.random.manual_seed(42)

model = CenterNetHourglass
loss = CenterNetLoss(0.1, 0.1, focal=focalLoss, regression=L1LossMask)
modelParams = {}
evaluation = centerNetEvaluation
