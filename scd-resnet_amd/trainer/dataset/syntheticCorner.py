"""Synthetic corner dataset plugin for CornerNet (config 4).  The reference ships no dataset
with corner targets (cornerNetCPool.py:43 imports a module that does not exist); its loss reads
ys[0] = centre heatmap, ys[3] = top-left heatmap, ys[4] = bottom-right heatmap
(cornerNetCPool.py:244-272).  Samples come from syntheticSCD; the corner of each object is its
centre -/+ (round |major_x|, round minor) clipped to the map, rendered with the same Gaussian
rule as the centre (tests/golden/make_golden_corner.py:corner_targets builds F8 the same way).

  __getitem__ -> {"xs": [tile (1,512,512) f32], "ys": [heat, mask (30,), regr (30,6), tl, br]}
  gpu_batch(indices, device) -> the same stacked, the three maps rendered on the GPU in one launch
                                (scd_render_corner_targets); the training loop's route
With the configuration key "cornerEmbeddings" on, ys grows by [tl_inds (30,) i64, br_inds, valid (30,) bool]: the
corner cells and slots cornerNetAE's embedding loss gathers its tags at (scd_corner_tag_inds).
"""
import numpy as np
import torch

from trainer.dataset.syntheticSCD import HEATMAPSIZE, MAXTAGLEN, SCD, encode_targets


def corner_locs(locs, size=HEATMAPSIZE):
    tl, br = locs.copy(), locs.copy()
    dx = np.round(np.abs(locs[:, 4])).astype(np.float32)
    dy = np.round(locs[:, 6]).astype(np.float32)
    tl[:, 0] = np.clip(locs[:, 0] - dx, 0, size - 1)
    tl[:, 1] = np.clip(locs[:, 1] - dy, 0, size - 1)
    br[:, 0] = np.clip(locs[:, 0] + dx, 0, size - 1)
    br[:, 1] = np.clip(locs[:, 1] + dy, 0, size - 1)
    return tl, br


def corner_tag_inds(locs, size=HEATMAPSIZE, K=MAXTAGLEN):
    """The host statement of scdhip.ops.corner_tag_inds for one sample's rows: (tl_inds, br_inds (K,) int64 = y * size
    + x of the corner cells of corner_locs, valid (K,) bool: the centre's cell on the map and both corners finite;
    0 / False for the other slots)."""
    tl_inds, br_inds, valid = np.zeros(K, np.int64), np.zeros(K, np.int64), np.zeros(K, bool)
    locs = locs[:K]
    tl, br = corner_locs(locs, size)
    with np.errstate(invalid="ignore"):
        cx, cy = np.trunc(locs[:, 0]), np.trunc(locs[:, 1])
        ok = (cx >= 0) & (cx < size) & (cy >= 0) & (cy < size) & np.isfinite(tl[:, :2]).all(1) & np.isfinite(br[:, :2]).all(1)
    for k in np.nonzero(ok)[0]:
        tl_inds[k] = int(tl[k, 1]) * size + int(tl[k, 0])
        br_inds[k] = int(br[k, 1]) * size + int(br[k, 0])
    valid[:len(locs)] = ok
    return tl_inds, br_inds, valid


def _embeddings():
    from configuration import defaultConfig
    return defaultConfig.cornerEmbeddings


class CornerSCD(SCD):
    def item(self, index, base):
        tile, locs, ys = super().item(index, base)
        tl, br = corner_locs(locs, self.heat)
        ys = ys[:3] + [torch.from_numpy(encode_targets(tl, self.heat)[0]),
                       torch.from_numpy(encode_targets(br, self.heat)[0])]
        if _embeddings():       # configuration key cornerEmbeddings: the cells and slots of the embedding loss
            ys += [torch.from_numpy(a) for a in corner_tag_inds(locs, self.heat)]
        return tile, locs, ys

    def gpu_batch(self, indices, device):
        """SCD.gpu_batch with the corner layout: the same tiles, the three maps from one launch of
        scd_render_corner_targets -> {"xs": [(B,1,S,S)], "ys": [heat, mask, regr, tl, br]} on `device`, equal to
        stacking __getitem__(i) for i in indices (tests/test_corner_targets_gpu.py)."""
        from scdhip import ops
        from trainer.dataset.syntheticSCD import THRESHOLDIOU
        tiles, locs, counts = self.batch_rows(indices)
        locs, counts = locs.to(device), counts.to(device)
        ys = ops.render_corner_targets(locs, counts, self.heat, THRESHOLDIOU)[:5]
        if _embeddings():
            ys += list(ops.corner_tag_inds(locs, counts, self.heat))
        return {"xs": [tiles.to(device)], "ys": ys}

    def getValidationSet(self, batch=None):
        from configuration import defaultConfig
        from trainer.dataset.syntheticSCD import VALID_SAMPLES
        batch = batch or min(VALID_SAMPLES, defaultConfig.validationBatchSize)
        out = []
        for b0 in range(0, VALID_SAMPLES, batch):
            items = [self.item(i, self.seed + 7919 * 1000003) for i in range(b0, min(VALID_SAMPLES, b0 + batch))]
            out.append({"xs": [torch.stack([it[0] for it in items])],
                        "ys": [torch.stack([it[2][k] for it in items]) for k in range(len(items[0][2]))]})
        return out


dataset = CornerSCD
