"""preprocess.py's host side and the scdx{N}p{M} dataset family, CPU only, against the reference's own output
(tests/golden/preproc.npz, tests/golden/make_golden_preproc.py): the label maths of datasets.preprocessor.scdManual
(decode, the 8-fold box replication, rotateCoordinates, the tile assignment), the command line, the 25 plugin
modules' constants and their split rule.

Label tolerance: per-tile object counts exact (the fixture's maker asserts that no centre lies within 1e-3 px of a
tile boundary); values within 1e-4 -- about ten float32 roundings of coordinates below 64 (64 * 2^-24 * 10 = 4e-5)."""
import importlib
import json
import random

import numpy as np
import pytest
import torch.utils.data

from oracle import scd_archive

# the reference's three constants per plugin (datasets/scds/scdx{N}p{M}.py:57-60)
FAMILY = {"scdx%dp%d" % (n, m): (n, p, "train%dp%d" % (n, m))
          for n in (1, 4, 8, 12, 16) for m, p in ((5, 0.05), (10, 0.10), (25, 0.25), (50, 0.50), (100, 1.00))}


@pytest.fixture(scope="module")
def fixture(golden):
    g = golden("preproc")
    names = [n[:-len(".npy")] for n in json.loads(bytes(g["names_json"]).decode())["names"]]
    ends = np.cumsum(g["locs_count"])
    locs = [g["locs"][e - c:e] for e, c in zip(ends, g["locs_count"])]
    return g, names, locs


def test_label_chain_matches_reference(fixture):
    from datasets.preprocessor import scdManual as M
    g, names, ref = fixture
    rows = M.decodeLines(bytes(g["annotation"]).decode().splitlines(True))
    assert len(rows) == 2
    H, W = g["slide"].shape[:2]
    assert len(M.replicateBoxes(rows, W, H)) == 18
    k = 0
    for angle in g["angles"]:
        tiles = M.tileLocs(rows, W, H, g["margin"].tolist(), int(g["tile"]), float(angle))
        assert len(tiles) == 12
        for got in tiles:
            assert got.dtype == np.float32 and got.shape == (len(ref[k]), 8), names[k]
            np.testing.assert_allclose(got, ref[k], rtol=0, atol=1e-4, err_msg=names[k])
            k += 1
    assert k == 192 and sum(len(l) for l in ref) > 16        # every repeat places objects
    assert len(rows[0]) == 8 and rows[0][0] == (9.5 + 19.0) / 2 // 4   # the decoded rows are left untouched


def test_decode_reads_the_annotation_file(tmp_path, fixture):
    from datasets.preprocessor import scdManual as M
    g = fixture[0]
    text = bytes(g["annotation"]).decode()
    (tmp_path / "7.txt").write_text(text + "\n")
    rows = M.decode(str(tmp_path) + "/", "7.png", 56, 40)
    assert rows == M.decodeLines(text.splitlines(True)) and len(rows) == 2
    cx, cy, ox, oy, majx, majy, minl, halo = rows[0]
    assert (cx, cy, ox, oy) == (3.0, 2.0, 2.25, 1.875)
    assert (majx, majy, minl, halo) == (9.5 / 8, 5.25 / 8, 3.0 / 8, 6.0 / 4)
    assert M.decode(str(tmp_path) + "/", "8.png", 56, 40) is None


def test_rotate_coordinates_rule():
    """A quarter turn about (xh - 0.5, yh - 0.5): centre, offset and major axis turn together; a zero offset stays
    zero (the reference's modMask)."""
    import torch

    from datasets.preprocessor import scdManual as M
    locs = torch.tensor([[10.0, 4.0, 0.0, 0.0, 2.0, 0.0, 1.0, 3.0], [3.0, 9.0, 1.0, 0.5, 0.0, -2.0, 1.0, 3.0]])
    out = M.rotateCoordinates(locs.clone(), 7, 5, 90.0).numpy()
    want = np.array([[6.5 - 0.5, 4.5 - 3.5, 0, 0, 0, -2, 1, 3], [6.5 + 4.5, 4.5 + 3.5, 0.5, -1, -2, 0, 1, 3]])
    np.testing.assert_allclose(out, want, rtol=0, atol=1e-5)


def test_angles_follow_the_reference_draws(fixture):
    g = fixture[0]
    np.random.seed(42)
    draws = [np.random.uniform() * 30 - 15 for _ in range(16)]
    np.testing.assert_array_equal(draws, g["angles"])


def test_fixture_naming_rule(fixture):
    """"<image>.<repeat>.<id>": 12 x-major tiles per repeat, the id running on across the repeats."""
    _, names, _ = fixture
    assert names == ["1.%d.%d" % (r, r * 12 + k + 1) for r in range(16) for k in range(12)]


def test_parser_defaults_and_margin():
    import preprocess as P
    a = P.parseArguments(["out.d"])
    assert (a.outputZipPath, a.inputImage, a.annotation, a.destinationSize, a.iouThreshold, a.verbal, a.margin,
            a.profile) == ("out.d", None, None, 512, 0.7, False, "0 0 0 0", None)
    a = P.parseArguments(["o.d", "-i", "im/", "-a", "an/", "-s", "256", "-t", "0.5", "-v", "-m", "64 32 16 8", "-p",
                          "datasets.preprocessor.scdManual"])
    s = P.settingsOf(a)
    assert s == {"outputPath": "o.d", "inputImage": "im/", "annotation": "an/", "destinationSize": 256,
                 "margin": [64, 32, 16, 8], "iouThreshold": 0.5, "verbal": True,
                 "profile": "datasets.preprocessor.scdManual"}
    assert P.settingsOf(P.parseArguments(["o.d"]))["margin"] == [0, 0, 0, 0]
    assert callable(importlib.import_module(s["profile"]).generateArchieve)


def test_generate_archive_needs_a_gpu(monkeypatch):
    import torch

    from datasets.preprocessor import scdManual as M
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.generateArchieve({"destinationSize": 16, "margin": [0, 0, 0, 0]}, [], None)


@pytest.mark.parametrize("name", sorted(FAMILY))
def test_family_constants(name):
    mod = importlib.import_module("trainer.dataset." + name)
    assert (mod.ARGUMENTRATIO, mod.PARTITION, mod.TRAINSUBSET) == FAMILY[name]
    assert mod.dataset is mod.SCD and mod.SCD.__module__ == mod.__name__
    assert (mod.SCD.ARGUMENTRATIO, mod.SCD.PARTITION, mod.SCD.TRAINSUBSET) == FAMILY[name]
    assert callable(mod.splitOrder) and callable(mod.readArchive) and callable(mod.writeArchive)
    assert (mod.TESTSET, mod.MAXTAGLEN, mod.HEATMAPSIZE) == (5760, 30, 128)


def test_family_has_the_reference_config_names():
    """The dataset names of the reference's configs/exp79..86.json."""
    for n in ("scdx8p100", "scdx12p100", "scdx4p100", "scdx1p100", "scdx16p50", "scdx16p25", "scdx16p10", "scdx16p5"):
        mod = importlib.import_module("trainer.dataset." + n)      # what train.py does with the config's name
        assert mod.TRAINSUBSET == "train" + n[len("scdx"):] and issubclass(mod.dataset, torch.utils.data.Dataset)


def test_split_x8p50_without_profile(golden):
    from trainer.dataset import scdx8p50 as D
    g = golden("preproc")
    random.seed(77)
    order, profile = D.splitOrder(scd_archive.CANONICAL, None)
    assert len(g["x8p50_valid"]) == 5760 and len(g["x8p50_train"]) == 49920 // 2 // 2 - 5760
    np.testing.assert_array_equal(profile["validation"], g["x8p50_valid"])
    np.testing.assert_array_equal(order, g["x8p50_train"])
    assert json.loads(json.dumps(profile)) == json.loads(bytes(g["x8p50_profile_json"]).decode())


def test_split_x1p5_with_profile(golden):
    from trainer.dataset import scdx1p5 as D
    g = golden("preproc")
    valid = golden("scd")["valid_ids"].tolist()
    random.seed(77)
    order, profile = D.splitOrder(scd_archive.CANONICAL, {"validation": valid})
    np.testing.assert_array_equal(profile["validation"], g["x1p5_valid"])
    np.testing.assert_array_equal(order, g["x1p5_train"])
    assert sorted(profile) == ["train1p5", "validation"] and profile["train1p5"] is order
    assert json.loads(json.dumps(profile)) == json.loads(bytes(g["x1p5_profile_json"]).decode())
    assert all((i // 24) % 16 < 1 for i in order) and not set(order) & set(valid)


def test_split_can_leave_no_training_tiles():
    """Without a profile the first TESTSET positions of the cut order are the validation set, whatever is left."""
    from trainer.dataset import scdx1p5 as D
    random.seed(3)
    order, profile = D.splitOrder(scd_archive.CANONICAL, None)
    assert order == [] and profile["train1p5"] == [] and len(profile["validation"]) == int(130 * 24 * 0.05)


def test_scdx16p100_split_unchanged(golden):
    from trainer.dataset import scdx16p100 as D
    g = golden("scd")
    assert (D.ARGUMENTRATIO, D.PARTITION, D.TRAINSUBSET) == (16, 1.0, "train16p100")
    random.seed(77)
    order, profile = D.splitOrder(scd_archive.CANONICAL, None)
    np.testing.assert_array_equal(profile["validation"], g["valid_ids"])
    np.testing.assert_array_equal(order, g["train_ids"])
