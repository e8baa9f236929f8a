"""cornerNetAE without a GPU: the configuration key, the conditions the golden fixture was drawn under
(tests/golden/make_golden_ae.py), the plugin's surface and the ctypes declarations of the new entry points."""
import os
import re

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRY_POINTS = ("scd_corner_tag_inds", "scd_corner_ae_fwd", "scd_corner_ae_bwd", "scd_corner_pairs")


def test_configuration_key_defaults_to_off():
    from configuration import Configuration
    c = Configuration()
    assert c.config["cornerEmbeddings"] is False and c.cornerEmbeddings is False
    c.updateConfig({"cornerEmbeddings": True})
    assert c.cornerEmbeddings is True


def test_fixture_conditions(golden):
    f = golden("ae")
    for case in ("mixed", "equal", "single"):
        mask = f["loss|%s|mask" % case]
        assert mask.dtype == np.uint8
        assert (mask.sum(1) >= 2).any()
        assert f["loss|%s|push64" % case] > 0 and f["loss|%s|push32" % case] > 0, case
    assert f["loss|mixed|mask"].sum(1).tolist() == [5, 1, 0, 8] and f["loss|single|mask"].shape[0] == 1
    tl, br = f["loss|equal|tl"], f["loss|equal|br"]
    assert tl[0, 1] == tl[0, 3] and br[0, 1] == br[0, 3]
    for case, K, count in (("small", 8, 64), ("large", 100, 1000)):
        det = f["pair|%s|det" % case]
        assert det.shape == (2, min(count, K * K), 8) and int(f["pair|%s|K" % case]) == K
        for b in range(2):
            v = det[b, :, 4][det[b, :, 4] >= 0]
            assert len(np.unique(v)) == len(v), (case, b)
            assert len(v) == f["pair|%s|nvalid" % case][b]
    assert f["pair|small|nvalid"][1] == 0
    assert f["pair|large|nall"][0] > 1000 > f["pair|large|nall"][1] > 0


def test_plugin_imports_and_loss_names_the_key_on_a_five_entry_layout():
    import trainer.model.cornerNetAE as plugin
    from models.cornerNetAE import CornerNetAEResidual, cornerNetAEEvaluation, expression
    assert plugin.model is CornerNetAEResidual and plugin.evaluation is cornerNetAEEvaluation
    assert plugin.expression is expression and plugin.modelParams == {"numLayers": 10}
    outs = [{k: torch.zeros(1, 1, 4, 4) for k in ("heatmap", "tl", "br", "tlTag", "brTag")}]
    ys = [torch.zeros(1, 1, 4, 4), torch.zeros(1, 3, dtype=torch.bool), torch.zeros(1, 3, 6), torch.zeros(1, 1, 4, 4),
          torch.zeros(1, 1, 4, 4)]
    with pytest.raises(RuntimeError, match="cornerEmbeddings"):
        plugin.loss(outs, ys)
    line = expression([])
    for field in ("[Obj]", "[Det]", "[mIoU]", "[Rec50]", "[Rec75]", "[Prec50]"):
        assert field in line


def test_model_state_dict_extends_cornernetcpool():
    from models.cornerNetAE import CornerNetAEResidual
    from models.cornerNetCPool import CornerNetResidual
    torch.manual_seed(11)
    sb = CornerNetResidual(10).state_dict()
    torch.manual_seed(11)
    sa = CornerNetAEResidual(10).state_dict()
    assert list(sa)[:len(sb)] == list(sb) and len(sa) == len(sb) + 8
    assert all(torch.equal(v, sa[k]) for k, v in sb.items())


def test_evaluation_counts_on_the_cpu():
    """The hook is plain torch: one object, one exact detection, one detection elsewhere, one below the score."""
    from models.cornerNetAE import box_iou, cornerNetAEEvaluation, expression
    W = 16
    ys = [torch.zeros(1, 1, W, W)] * 5 + [torch.tensor([[2 * W + 1, 0]]), torch.tensor([[9 * W + 6, 0]]),
                                          torch.tensor([[True, False]])]
    det = torch.tensor([[[1., 2, 6, 9, 0.9, 0, 0, 0], [10, 10, 12, 12, 0.5, 0, 0, 0], [1, 2, 6, 9, 0.1, 0, 0, 0],
                         [0, 0, 0, 0, -1, 0, 0, 0]]])
    c = cornerNetAEEvaluation(None, ys, det, None)[0]["counts"].tolist()
    assert c == [1, 2, 1, 1, 1, 1]
    assert "[Prec50] 50.00" in expression([{"counts": torch.tensor(c)}])
    a = torch.tensor([[[0., 0, 3, 3]]])
    assert box_iou(a, torch.tensor([[[2., 2, 5, 5]]])).item() == pytest.approx(4 / 28)


def test_lib_declares_the_new_entry_points_with_the_headers_argument_counts():
    import scdhip.lib as L
    src = open(os.path.join(REPO, "include", "scdhip.h")).read()
    for name in NEW_ENTRY_POINTS:
        m = re.search(r"^int %s\((.*?)\);" % name, src, re.M | re.S)
        assert m, name
        assert name in L.SIGNATURES, name
        res, args = L.SIGNATURES[name]
        assert res is L.c_int and len(args) == len(m.group(1).split(",")), name
