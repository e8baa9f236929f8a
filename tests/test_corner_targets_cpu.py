"""CornerNet training end to end, host side, CPU only: the configuration key, the dataset overrides, the
loss' guard and the validation counts of cornerNetEvaluation / expression against numpy."""
import importlib
import re

import numpy as np
import pytest
import torch


def test_corner_targets_key_defaults_off_and_follows_update():
    from configuration import Configuration, defaultConfig
    assert defaultConfig.cornerTargets is False
    c = Configuration()
    assert c.config["cornerTargets"] is False and c.cornerTargets is False
    c.updateConfig({"cornerTargets": True})
    assert c.cornerTargets is True
    c.updateConfig({"cornerTargets": False})
    assert c.cornerTargets is False


def test_corner_dataset_overrides_gpu_batch():
    from trainer.dataset import syntheticCorner, syntheticSCD
    assert syntheticCorner.CornerSCD.gpu_batch is not syntheticSCD.SCD.gpu_batch
    assert "gpu_batch" in vars(syntheticCorner.CornerSCD)
    # the routes bench.py and the existing tests read stay the class's own
    assert syntheticCorner.CornerSCD.__getitem__ is syntheticSCD.SCD.__getitem__
    assert syntheticCorner.dataset is syntheticCorner.CornerSCD


def test_all_25_plugins_still_share_one_gpu_batch():
    from trainer.dataset import scdx16p100 as D
    mods = [importlib.import_module("trainer.dataset.scdx%dp%d" % (n, m))
            for n in (1, 4, 8, 12, 16) for m in (5, 10, 25, 50, 100)]
    assert len(mods) == 25
    for mod in mods:
        assert mod.SCD.gpu_batch is D.SCD.gpu_batch and mod.SCD._resident_batch is D.SCD._resident_batch
        assert mod.SCD._buildValidation is D.SCD._buildValidation
        assert mod.SCD.getValidationSet is D.SCD.getValidationSet


def test_loss_names_the_key_for_a_centernet_target_list():
    from trainer.model.cornerNetCPool import loss
    maps = {k: torch.zeros(2, 1, 8, 8) for k in ("heatmap", "tl", "br")}
    heat = torch.zeros(2, 1, 8, 8)
    four = [heat, torch.zeros(2, 30, dtype=torch.bool), torch.zeros(2, 30, 6), torch.zeros(2, 30, dtype=torch.int64)]
    with pytest.raises(RuntimeError, match="cornerTargets") as e:
        loss([maps], four)
    assert "syntheticCorner" in str(e.value)
    # five entries, but not maps: the CenterNet validation layout's locs rows and object counts
    with pytest.raises(RuntimeError, match="cornerTargets"):
        loss([maps], four[:3] + [torch.zeros(2, 30, 8), torch.zeros(2, 30, dtype=torch.int64)])
    with pytest.raises(RuntimeError, match="cornerTargets"):
        loss([maps], four[:3] + [heat, heat.long()])


def test_validation_without_corner_maps_raises():
    """A dataset built with the key off holds no corner maps: asking for the corner layout says so."""
    from configuration import defaultConfig
    from trainer.dataset import scdx16p100 as D
    ds = object.__new__(D.SCD)
    ds.validation = {"xs": [None, None], "ys": [None] * 5}
    old = dict(defaultConfig.config)
    defaultConfig.config["cornerTargets"] = True
    try:
        with pytest.raises(RuntimeError, match="cornerTargets was off"):
            ds.getValidationSet()
    finally:
        defaultConfig.config.clear()
        defaultConfig.config.update(old)


def _decode_case(rs):
    """A hand-built decodeCornerNet result for 2 images, K = 4 on 8 x 8 maps, and its ground truth.  Per map the four
    detections of image 0 sit on ground-truth values 0.8, 0.75, 0.6, 0.5 with the third below the score threshold;
    image 1 has values 0.74, 0.49, 1.0, 0.0 at random scores around 0.3."""
    N, K, S = 2, 4, 8
    ys = [None, torch.tensor([[True] * 3 + [False] * 27, [True] * 5 + [False] * 25]), torch.zeros(N, 30, 6), None, None]
    decoded = []
    values = np.array([[0.8, 0.75, 0.6, 0.5], [0.74, 0.49, 1.0, 0.0]], np.float32)
    for m in (0, 3, 4):
        gt = np.full((N, 1, S, S), 0.25, np.float32)
        cells = np.stack([rs.choice(S * S, K, replace=False) for _ in range(N)])
        cy, cx = cells // S, cells % S
        for n in range(N):
            gt[n, 0, cy[n], cx[n]] = values[n]
        scores = rs.uniform(0.31, 1.0, (N, K)).astype(np.float32)
        scores[0, 2] = 0.29                                             # below 0.3: counted nowhere
        scores[1] = np.float32([0.3, 0.2999, 0.9, 0.5])                 # exactly on the threshold counts
        ys[m] = torch.from_numpy(gt)
        decoded += [torch.from_numpy(scores), torch.from_numpy(cells), torch.from_numpy(cy), torch.from_numpy(cx)]
    return ys, decoded + [{}]


def _numpy_hits(ys, decoded):
    out = np.zeros((3, 3), np.int64)
    for m, k in enumerate((0, 3, 4)):
        gt = ys[k].numpy()
        s, _, cy, cx = [d.numpy() for d in decoded[4 * m:4 * m + 4]]
        for n in range(s.shape[0]):
            for j in range(s.shape[1]):
                if s[n, j] >= np.float32(0.3):
                    v = gt[n, 0, cy[n, j], cx[n, j]]
                    out[m] += [1, v >= 0.5, v >= 0.75]
    return out


def test_evaluation_counts_and_expression_against_numpy():
    from trainer.model import cornerNetCPool as plugin
    assert plugin.expression.__module__ == "models.cornerNetCPool"
    rs = np.random.RandomState(3)
    total, batches = np.zeros((3, 3), np.int64), []
    for _ in range(2):
        ys, decoded = _decode_case(rs)
        ev, out = plugin.evaluation([None], ys, *decoded)
        assert out is decoded[-1] and set(ev) == {"objs", "scores", "valid", "hits"}
        assert ev["objs"] == [3, 5] and torch.equal(ev["valid"], decoded[0] >= 0.3)
        assert ev["hits"].dtype == torch.int64 and ev["hits"].shape == (3, 3)
        want = _numpy_hits(ys, decoded)
        np.testing.assert_array_equal(ev["hits"].numpy(), want)
        np.testing.assert_array_equal(want, [[6, 5, 3]] * 3)      # 0.29 and 0.2999 dropped; 0.5 and 0.75 count
        total += want
        batches.append(ev)
    text = plugin.expression(batches)
    assert re.search(r"\[Obj\]\s+16\b", text)
    for name, (det, h50, h75) in zip(("Ct", "TL", "BR"), total):
        assert re.search(r"\[%s\]\s+%d\b" % (name, det), text), text
        assert "[%shit50] %s" % (name, format(100.0 * h50 / det, "-5.2f")) in text
        assert "[%shit75] %s" % (name, format(100.0 * h75 / det, "-5.2f")) in text
    assert "83.33" in text and "50.00" in text
    # no detection at all: zeros, no division
    ys, decoded = _decode_case(rs)
    for m in range(3):
        decoded[4 * m] = torch.zeros(2, 4)
    ev, _ = plugin.evaluation([None], ys, *decoded)
    assert not ev["hits"].any()
    empty = plugin.expression([ev])
    assert re.search(r"\[TL\]\s+0\b", empty) and re.search(r"\[TLhit50\]\s+0\.00\b", empty)
    assert "[Ct]" in plugin.expression([]) and "[BR]" in plugin.expression([])
