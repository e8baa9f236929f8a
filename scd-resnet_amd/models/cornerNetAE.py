"""CornerNet that outputs boxes: cornerNetCPool's ResNet / CornerPool model with the two embedding-tag heads, the
associative-embedding loss and the corner pairing decode of the reference's hourglass CornerNet
(models/cornerNetLegacy.py: tag heads :262, CornerNetLoss :558-640, decodeCornerNet :332-446;
models/losses/embeddings.py), none of which needs the hourglass.  DESIGN §8f.

The tag heads are plain tails (Conv3x3 256->128 + bias, ReLU, Conv1x1 128->1) that read the same CornerPool output
as their corner's heat tail, so each corner runs one CornerPoolFn and one two-head HeadsFn (the fused heads GEMM);
the tag heads' output gradient lives on the gathered cells only and takes the sparse heads backward.
"""
import torch

from models.cornerNetCPool import HIT_SCORE, CornerNetResidual, makeResnetTerminal
from models.losses.focal import focalLoss
from scdhip import blocks, ops
from scdhip.loss import CornerNetAELossFn

OUTPUTS = ("heatmap", "tl", "br", "tlTag", "brTag")
IOU_LEVELS = (0.5, 0.75)


class CornerNetAEResidual(CornerNetResidual):
    """CornerNetResidual's module tree and state-dict keys, then `tlTag` and `brTag`: created after every inherited
    module and its initialisation, so one seed gives the inherited parameters CornerNetResidual's initial values.
    The tag tails keep torch's default initialisation."""

    def __init__(self, numLayers):
        super(CornerNetAEResidual, self).__init__(numLayers)
        self.decoder = decodeCornerNetAE
        self.tlTag = makeResnetTerminal(self.prediction, 128, 1)
        self.brTag = makeResnetTerminal(self.prediction, 128, 1)

    def heads_forward(self, feat, *x, **kwargs):
        ops.share_grad(feat, 3)             # the heatmap head and the two CornerPools
        ret = {"heatmap": blocks.HeadsFn.apply(feat, self.heatmap[0].weight, [self.heatmap])[0]}
        for name, tag in (("tl", "tlTag"), ("br", "brTag")):
            m, t = getattr(self, name), getattr(self, tag)
            h = blocks.CornerPoolFn.apply(feat, m[0].branch1.conv.weight, m[0], m[0].dirs)
            ret[name], ret[tag] = blocks.HeadsFn.apply(h, m[1].weight, [(m[1], m[2], m[3]), t])
        return {n: ret[n] for n in OUTPUTS}


class CornerNetAELoss(torch.nn.Module):
    """focal(heatmap, ys[0]) + focal(tl, ys[3]) + focal(br, ys[4]) + pullWeight * pull + pushWeight * push, the tags
    gathered at ys[5] / ys[6] where ys[7] (cornerNetLegacy.py:558-640 with one output stack and no regression heads;
    weights 1 and 1 as :560)."""

    def __init__(self, pullWeight=1, pushWeight=1, focal=focalLoss):
        super(CornerNetAELoss, self).__init__()
        self.pullWeight, self.pushWeight, self.focal = pullWeight, pushWeight, focal

    def forward(self, outs, targets):
        if self.focal is not focalLoss or len(outs) != 1:
            raise NotImplementedError("fused HIP focal loss over one output stack")
        t = targets
        if (len(t) != 8 or not all(torch.is_tensor(t[k]) and t[k].is_floating_point() and t[k].shape == t[0].shape
                                   for k in (0, 3, 4))
                or not all(torch.is_tensor(t[k]) and t[k].dim() == 2 and t[k].shape == t[5].shape for k in (5, 6, 7))):
            raise RuntimeError("CornerNetAELoss needs the embedding layout [heat, mask, regr, tl, br, tl_inds, br_inds, "
                               "valid], got %d targets: train cornerNetAE on the `syntheticCorner` dataset or on a `.d` "
                               "plugin with the configuration keys \"cornerTargets\": true and "
                               "\"cornerEmbeddings\": true" % len(t))
        o = outs[0]
        loss, stats = CornerNetAELossFn.apply(o["heatmap"], o["tl"], o["br"], o["tlTag"], o["brTag"], t[0], t[3], t[4],
                                              t[5], t[6], t[7], self.pullWeight, self.pushWeight)
        self.last_stats = stats     # device tensor [focal heat, focal tl, focal br, pull, push]; no host read here
        return loss, {}


def decodeCornerNetAE(outputDictionary, K=100, nmsKernelSize=3, threshold=1.0, count=1000, **kwargs):
    """[det (N,D,8), nvalid (N,), ct scores/inds/ys/xs, outputDictionary]: decode_topk on the three maps, then the
    corner pairing (ops.corner_pairs).  det rows are the reference's [x_tl, y_tl, x_br, y_br, score, s_tl, s_br, 0]."""
    if nmsKernelSize != 3:
        raise NotImplementedError("3x3 NMS")
    od = outputDictionary
    ct, tl, br = (ops.decode_topk(od[key], None, None, K)[:4] for key in ("heatmap", "tl", "br"))
    det, nvalid = ops.corner_pairs(tl, br, od["tlTag"], od["brTag"], threshold, count)
    return [det, nvalid, *ct, outputDictionary]


def box_iou(a, b):
    """IoU of boxes a (N,A,4) and b (N,B,4) -> (N,A,B).  Boxes are [x0, y0, x1, y1] in cells, both corner cells
    included (a box whose corners share a cell has area 1)."""
    a, b = a[:, :, None, :], b[:, None, :, :]
    iw = (torch.minimum(a[..., 2], b[..., 2]) - torch.maximum(a[..., 0], b[..., 0]) + 1).clamp(min=0)
    ih = (torch.minimum(a[..., 3], b[..., 3]) - torch.maximum(a[..., 1], b[..., 1]) + 1).clamp(min=0)
    inter = iw * ih
    area = lambda t: (t[..., 2] - t[..., 0] + 1) * (t[..., 3] - t[..., 1] + 1)      # noqa: E731
    return inter / (area(a) + area(b) - inter)


def cornerNetAEEvaluation(xs, ys, *decoded):
    """Validation hook: plain torch on the device, no host read.  Ground-truth boxes are the cells of ys[5] / ys[6]
    where ys[7]; a detection is a row of det with score >= HIT_SCORE.  Returns {"counts": float64 (6,) = [objects,
    detections, sum over objects of the best IoU among the detections, objects with best IoU >= 0.5, >= 0.75,
    detections whose best IoU with any object is >= 0.5]}.  These counts are this project's (the reference's hook calls
    an averagePrecision it does not ship): no reference metric, and no accuracy claim."""
    det, outputDictionary = decoded[0], decoded[-1]
    tl_inds, br_inds, valid = ys[5], ys[6], ys[7].bool()
    W = ys[0].shape[-1]
    gt = torch.stack([tl_inds % W, tl_inds // W, br_inds % W, br_inds // W], -1).float()
    isdet = det[..., 4] >= HIT_SCORE
    pair = valid[:, :, None] & isdet[:, None, :]
    iou = torch.where(pair, box_iou(gt, det[..., :4]), torch.zeros((), device=det.device))
    best_obj = iou.amax(2) if iou.shape[2] else iou.new_zeros(iou.shape[:2])       # (N,K): 0 without detections
    best_det = iou.amax(1) if iou.shape[1] else iou.new_zeros(iou.shape[0], iou.shape[2])
    counts = torch.stack([valid.sum().double(), isdet.sum().double(), (best_obj * valid).sum().double()]
                         + [(valid & (best_obj >= lv)).sum().double() for lv in IOU_LEVELS]
                         + [(isdet & (best_det >= IOU_LEVELS[0])).sum().double()])
    return {"counts": counts.detach()}, outputDictionary


def expression(batches):
    """The evals line of a validation pass: the counts summed over the batches, read once."""
    c = torch.stack([b["counts"] for b in batches]).sum(0).tolist() if batches else [0.0] * 6
    obj, det, siou, r50, r75, p50 = c
    return ("[Obj] {:7d}    [Det] {:7d}    [mIoU] {:6.4f}    [Rec50] {:5.2f}    [Rec75] {:5.2f}    [Prec50] {:5.2f}"
            .format(int(obj), int(det), siou / obj if obj else 0.0, 100.0 * r50 / obj if obj else 0.0,
                    100.0 * r75 / obj if obj else 0.0, 100.0 * p50 / det if det else 0.0))
