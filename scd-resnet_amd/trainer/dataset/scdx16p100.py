"""`.d` archive dataset plugin `scdx16p100` (datasets/scds/scdx16p100.py of the reference), and the
one implementation behind the 25 plugins `scdx{N}p{M}` of this package: the reference's
datasets/scds/scdx{1,4,8,12,16}p{5,10,25,50,100}.py differ in three constants only (ARGUMENTRATIO = N, how many of
the 16 preprocess rotations per slide to keep; PARTITION = M / 100, the share of the kept tiles to use; TRAINSUBSET =
'train{N}p{M}', the split profile's key), so each of the other 24 modules is `globals().update(family(N, M))`.  The
implementation stays in this module, which tests/golden/make_golden_scd.py loads by file path outside the package.

The on-disk format is the reference's (scdx16p100.py:64-93; written by preprocess.py:78-109 through a profile's
generateArchieve): a zip holding
    dataset.json          {"names": [name, ...]}
    object-count.json     {"count": {name: n, ...}}
    samples/<name>.npy    (H, W) grayscale tile
    locs/<name>.npy       (n, 8) float rows [ctx, cty, offx, offy, majx, majy, minl, halo] (heatmap units)
Constructor, split rules and sample format are the reference's:
  * samples index FSI x ARGUM x CLIP = 130 x 16 x 24 raw positions, kept when argum < ARGUMENTRATIO, shuffled with
    Python's `random` (unseeded, as the reference), cut to PARTITION (:143-158);
  * no split profile: the first TESTSET shuffled positions of that cut order become the validation set (even
    when that leaves no training tile), the rest TRAINSUBSET; with a profile: its TRAINSUBSET list, or the cut
    order minus its `validation` list, added to the profile under TRAINSUBSET (:160-180); the profile is written
    back to defaultConfig.dirDataSplitProfile (:264-266);
  * validation set: normalize (no augmentation), heat / mask / regr / locs / inds with the objects' centres
    truncated to integers (:188-262), served in validationBatchSize slices by getValidationSet (:381-414);
  * __getitem__(i): reshuffle at i == 0, x / y flips (numpy.random.uniform() > 0.5), normalize, variance jitter
    and Gaussian noise (0.05 each), targets (:300-379).
MI355X-native differences: the archive is read straight from the zip (no extraction into dirTemp; an already
extracted dirTemp/confocalCenter/ is still used when present); the tile augmentation runs as scd_augment_tiles
and the targets as scd_render_center_targets, batched over a whole training batch by gpu_batch() -- the
reference does both per sample in PyTorch.  Stored bounds are never mutated (the reference's CPU path flips
and truncates them in place, :424-429, :523-525).  A smaller-than-canonical archive (tests) indexes only the
positions it holds.  The reference's CUDA path pins cuda:0 (:316-356); here the device is the caller's.
The random-angle rotation the reference wrote as the augmentation's last step and left switched off (:443-486) runs
here when the configuration key rotateAugmentation (maximum absolute angle, degrees) is above 0: scd_rotate_tiles
on the augmented tiles, SCD.rotateLocs on the flipped labels; the validation set is never rotated.
With the configuration key residentDataset on, the first gpu_batch uploads the whole archive to the device (tiles as
one store, labels as CSR) and every batch is built there from the same host draws: scd_augment_tiles_indexed,
scd_rotate_tiles, scd_pack_locs (the flips, the rotation and the packing of the labels in one launch) and
scd_render_center_targets, without reading a host tile or label.  With the key off, the default,
nothing of this runs.
With the configuration key cornerTargets on, training batches (host and resident path) and validation slices carry
CornerNet's layout ys = [heat, mask, regr, tl, br]: scd_render_corner_targets renders the three maps from the same
packed rows in one launch, after the flips and the rotation; with the key off, the default, every route
is what it was.
"""
import io
import json
import os
import zipfile
from random import shuffle

import numpy as np
import torch
from torch.utils.data import Dataset

MAXTAGLEN = 30
TARGETSIZE = 512
HEATMAPSIZE = 128
THRESHOLDIOU = 0.5
TESTSET = 5760
REALTIMETEST = 5760
ARGUMENTRATIO = 16
PARTITION = 1.00
TRAINSUBSET = 'train16p100'
FSI, ARGUM, CLIP = 130, 16, 24
NOISESV, JITTERSV = 0.05, 0.05

__all__ = ["SCD", "dataset", "writeArchive", "readArchive", "splitOrder", "family"]
# what a family() plugin takes from this module as it stands, beside its own three constants, SCD / dataset and
# splitOrder: the reference modules' other constants and the archive functions
FAMILY_NAMES = ("MAXTAGLEN", "TARGETSIZE", "HEATMAPSIZE", "THRESHOLDIOU", "TESTSET", "REALTIMETEST", "FSI", "ARGUM",
                "CLIP", "NOISESV", "JITTERSV", "writeArchive", "readArchive")


def writeArchive(path, names, samples, locs):
    """Write a `.d` archive in the reference's layout (the generateArchieve contract of preprocess.py:99-105)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as z:
        z.writestr("dataset.json", json.dumps({"names": list(names)}))
        z.writestr("object-count.json", json.dumps({"count": {n: int(len(l)) for n, l in zip(names, locs)}}))
        for n, s, l in zip(names, samples, locs):
            for sub, arr in (("samples", s), ("locs", np.asarray(l, np.float32).reshape(-1, 8))):
                buf = io.BytesIO()
                np.save(buf, arr, allow_pickle=False)
                z.writestr("%s/%s.npy" % (sub, n), buf.getvalue())


def readArchive(zipPath, tempDir=None):
    """-> (names, objectCounts, samples [(1,H,W) f32 tensors], bounds [(n,8) f32 tensors]) (scdx16p100.py:98-135).
    Reads an extracted tempDir when it exists (the reference's cache), else the zip members directly."""
    if tempDir is not None and os.path.exists(tempDir):
        def read(name):
            with open(os.path.join(tempDir, name), "rb") as f:
                return f.read()
        z = None
    else:
        z = zipfile.ZipFile(zipPath)
        read = z.read
    try:
        names = json.loads(read("dataset.json"))["names"]
        counts = json.loads(read("object-count.json"))
        samples, bounds = [], []
        for n in names:
            s = np.load(io.BytesIO(read("samples/%s.npy" % n)), allow_pickle=False)
            l = np.load(io.BytesIO(read("locs/%s.npy" % n)), allow_pickle=False)
            samples.append(torch.from_numpy(np.ascontiguousarray(s)).unsqueeze(0).float())
            bounds.append(torch.from_numpy(np.ascontiguousarray(l, dtype=np.float32)).reshape(-1, 8))
    finally:
        if z is not None:
            z.close()
    return names, counts, samples, bounds


def _log(msg):
    try:
        from logger import Logger
        Logger.log(msg)
    except Exception:  # logging is cosmetic
        pass


def _device(useGPU):
    if not torch.cuda.is_available():
        raise RuntimeError("scdx16p100: the augmentation and target kernels run on MI355X only (no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


def _pack_locs(bounds_list, trunc):
    """(B, MAXTAGLEN, 8) rows + per-tile counts; trunc: centres truncated toward zero, as the reference's
    `loc[0] = int(loc[0])` before drawing (scdx16p100.py:201-202, :523-525)."""
    B = len(bounds_list)
    locs = np.zeros((B, MAXTAGLEN, 8), np.float32)
    counts = np.zeros(B, np.int32)
    for b, l in enumerate(bounds_list):
        l = (l.numpy() if torch.is_tensor(l) else np.asarray(l)).astype(np.float32)[:MAXTAGLEN]
        locs[b, :len(l)] = l
        counts[b] = len(l)
    if trunc:
        locs[:, :, :2] = np.trunc(locs[:, :, :2])
    return locs, counts


def _render_targets(locs, counts):
    """The targets of packed device rows: scd_render_center_targets' [heat, mask, regr, inds], or with the configuration
    key cornerTargets on scd_render_corner_targets' [heat, mask, regr, tl, br, inds] (the first four bit for bit the
    same)."""
    from configuration import defaultConfig
    from scdhip import ops
    if defaultConfig.cornerEmbeddings and not defaultConfig.cornerTargets:
        raise RuntimeError("scdx16p100: the configuration key cornerEmbeddings needs cornerTargets on")
    render = ops.render_corner_targets if defaultConfig.cornerTargets else ops.render_center_targets
    return render(locs, counts, HEATMAPSIZE, THRESHOLDIOU)


def _corner_layout(ys, locs, counts):
    """A training batch's ys from _render_targets' list: its first five entries, and with the configuration key
    cornerEmbeddings on the corner cells and slots of the same device rows behind them (scd_corner_tag_inds):
    [heat, mask, regr, tl, br, tl_inds, br_inds, valid]."""
    from configuration import defaultConfig
    if not defaultConfig.cornerEmbeddings:
        return ys[:5]
    from scdhip import ops
    return ys[:5] + list(ops.corner_tag_inds(locs, counts, HEATMAPSIZE))


def splitOrder(count, dataSplit=None, ratio=ARGUMENTRATIO, partition=PARTITION, subset=TRAINSUBSET):
    """Training order and split profile (scdx16p100.py:143-180): FSI x ARGUM x CLIP positions (only the first
    `count` of a smaller test archive) kept when argum < ratio, shuffled with Python's global `random`, cut to
    partition; then the split, the training ids under the profile's key `subset`.  Returns (order, dataProfile)."""
    total = min(FSI * ARGUM * CLIP, count)
    order = [i for i in range(total) if (i // CLIP) % ARGUM < ratio]
    shuffle(order)
    order = order[0: int(len(order) * partition)]
    if dataSplit is None:
        _log("The Data Split Profile Do Not Exist, We Randomly Select 10 pct. of Samples as Validation Set.")
        shuffle(order)
        numValidation = round(TESTSET)
        profile = {'validation': order[0:numValidation]}
        order = order[numValidation:]
        profile[subset] = order
    else:
        _log("Extracting Validation Set from Data Split Profile ...")
        profile = dataSplit
        if subset in profile.keys():
            order = profile[subset]
        else:
            valid = set(profile['validation'])
            order = [x for x in order if x not in valid]
            profile[subset] = order
    return order, profile


class SCD(Dataset):
    ARGUMENTRATIO, PARTITION, TRAINSUBSET = ARGUMENTRATIO, PARTITION, TRAINSUBSET

    def __init__(self, zipPath, useGPU, dataSplit=None):
        from configuration import defaultConfig
        tempDir = defaultConfig.dirTemp + 'confocalCenter' + "/"
        self.names, self.objectCounts, self.samples, self.bounds = readArchive(zipPath, tempDir)
        self.count = len(self.names)
        self.useGPU = useGPU
        self.device = _device(useGPU)

        self.order, self.dataProfile = splitOrder(len(self.names), dataSplit, ratio=self.ARGUMENTRATIO,
                                                  partition=self.PARTITION, subset=self.TRAINSUBSET)
        self.count = len(self.order)

        self._buildValidation()
        with open(defaultConfig.dirDataSplitProfile, "w+") as f:
            f.write(json.dumps(self.dataProfile))
        _log("Building Validation Set Completely with {} Samples".format(len(self.validObjNum)))

    # ------------------------------------------------------------------ validation (scdx16p100.py:185-262)
    def _buildValidation(self, chunk=256):
        from configuration import defaultConfig
        from scdhip import ops
        ids = self.dataProfile['validation'][:REALTIMETEST]
        xs, heat, mask, regr, locs, inds, tl, br, tags = [], [], [], [], [], [], [], [], ([], [], [])
        self.validObjNum = [int(len(self.bounds[i])) for i in ids]
        for c0 in range(0, len(ids), chunk):
            part = ids[c0:c0 + chunk]
            tiles = torch.stack([self.samples[i] for i in part]).to(self.device)
            xs.append(ops.augment_tiles(tiles))
            l, n = _pack_locs([self.bounds[i] for i in part], trunc=True)
            L = torch.from_numpy(l).to(self.device)
            h, m, r, *corners, ind = _render_targets(L, torch.from_numpy(n).to(self.device))
            for kept, c in zip((tl, br), corners):      # cornerTargets on
                kept.append(c)
            if defaultConfig.cornerEmbeddings:
                for kept, c in zip(tags, ops.corner_tag_inds(L, torch.from_numpy(n).to(self.device), HEATMAPSIZE)):
                    kept.append(c)
            # validation masks every stored object (scdx16p100.py:219-220)
            m = torch.arange(MAXTAGLEN, device=self.device)[None, :] < torch.from_numpy(n).to(self.device)[:, None]
            heat.append(h); mask.append(m); regr.append(r); locs.append(L); inds.append(ind)
        cat = (lambda ts, shape: torch.cat(ts) if ts else torch.zeros(shape, device=self.device))
        self.validation = {
            "xs": [cat(xs, (0, 1, 1, 1)), cat(inds, (0, MAXTAGLEN)).long()],
            "ys": [cat(heat, (0, 1, HEATMAPSIZE, HEATMAPSIZE)), cat(mask, (0, MAXTAGLEN)).bool(),
                   cat(regr, (0, MAXTAGLEN, 6)), cat(locs, (0, MAXTAGLEN, 8)), self.validObjNum]}
        if defaultConfig.cornerTargets:
            self.validation["corners"] = [cat(t, (0, 1, HEATMAPSIZE, HEATMAPSIZE)) for t in (tl, br)]
        if defaultConfig.cornerEmbeddings:
            self.validation["tags"] = [cat(t, (0, MAXTAGLEN)) for t in tags]

    def getValidationSet(self):
        """scdx16p100.py:381-414 (REALTIMETEST positions in validationBatchSize slices; empty slices of a small
        archive are dropped).  With the configuration key cornerTargets on every slice carries CornerNet's layout
        ys = [heat, mask, regr, tl, br], the corner maps _buildValidation kept; with cornerEmbeddings on too, the
        three (., K) tensors tl_inds, br_inds, valid behind them."""
        from configuration import defaultConfig
        v = self.validation
        length = REALTIMETEST
        size = defaultConfig.validationBatchSize
        if defaultConfig.cornerTargets:
            if "corners" not in v:
                raise RuntimeError("scdx16p100: cornerTargets was off when this dataset was built, its validation set "
                                   "holds no corner maps")
            extra = []
            if defaultConfig.cornerEmbeddings:
                if "tags" not in v:
                    raise RuntimeError("scdx16p100: cornerEmbeddings was off when this dataset was built, its "
                                       "validation set holds no corner cells")
                extra = v["tags"]
            part = (lambda s: [v['ys'][0][s], v['ys'][1][s], v['ys'][2][s], v['corners'][0][s], v['corners'][1][s]]
                    + [t[s] for t in extra])
        else:
            part = (lambda s: [v['ys'][0][s], v['ys'][1][s], v['ys'][2][s], v['ys'][3][s], v['ys'][4][s],
                               v['xs'][1][s]])
        if length > size:
            out = []
            for k in range(length // size):
                s = slice(int(k * size), int((k + 1) * size))
                if len(v['ys'][4][s]) == 0:
                    continue
                out.append({'xs': [v['xs'][0][s]], 'ys': part(s)})
            return out
        return [{'xs': [v['xs'][0]], 'ys': part(slice(None))}]

    # ------------------------------------------------------------------ training samples (scdx16p100.py:300-379)
    def __len__(self):
        return self.count

    @staticmethod
    def flipLocs(locs, fx, fy):
        """scdx16p100.py:424-436: mirrored centre, offset and major-axis components."""
        locs = (locs.numpy() if torch.is_tensor(locs) else np.asarray(locs)).astype(np.float32).reshape(-1, 8)
        if fx and len(locs):
            locs[:, 0] = HEATMAPSIZE - 1 - locs[:, 0]
            locs[:, 2] = -locs[:, 2]
            locs[:, 4] = -locs[:, 4]
        if fy and len(locs):
            locs[:, 1] = HEATMAPSIZE - 1 - locs[:, 1]
            locs[:, 3] = -locs[:, 3]
            locs[:, 5] = -locs[:, 5]
        return locs

    @staticmethod
    def rotateLocs(locs, angle, size=HEATMAPSIZE):
        """The label half of the rotation the reference holds switched off (scdx16p100.py:455-483): every row and
        its eight mirror images across the map's edges, in the reference's order (:459-471), turned by `angle`
        degrees about (size // 2 - 0.5, size // 2 - 0.5) with the reference's float32 rotateCoordinates (restated
        in datasets.preprocessor.scdManual), then the rows whose truncated centre (int(), toward zero) lies in
        [0, size) on both axes, in order.  One deviation: a centre at distance 0 from the rotation centre stays
        where it is (the reference divides 0 / 0 there and then fails in int(nan))."""
        from datasets.preprocessor.scdManual import rotateCoordinates
        locs = (locs.numpy() if torch.is_tensor(locs) else np.asarray(locs)).astype(np.float32).reshape(-1, 8)
        if not len(locs):
            return locs
        far = np.float32(2 * size - 1)
        rep = np.repeat(locs[:, None, :], 9, axis=1)
        ctx, cty = locs[:, 0], locs[:, 1]
        xs = (ctx, far - ctx, np.float32(-1) - ctx)
        ys = (cty, np.float32(-1) - cty, far - cty)
        for k in range(9):
            kx, ky = divmod(k, 3)
            rep[:, k, 0], rep[:, k, 1] = xs[kx], ys[ky]
            if kx:
                rep[:, k, 2], rep[:, k, 4] = -locs[:, 2], -locs[:, 4]
            if ky:
                rep[:, k, 3], rep[:, k, 5] = -locs[:, 3], -locs[:, 5]
        rep = rep.reshape(-1, 8)
        half = size // 2
        still = (rep[:, 0] + np.float32(0.5 - half) == 0) & (rep[:, 1] + np.float32(0.5 - half) == 0)
        out = rotateCoordinates(torch.from_numpy(rep.copy()), half, half, angle).numpy()
        out[still, :2] = rep[still, :2]
        cx, cy = np.trunc(out[:, 0]), np.trunc(out[:, 1])
        return out[(cx >= 0) & (cx < size) & (cy >= 0) & (cy < size)]

    def _draws(self, B):
        """The reference's random draws per sample, in its order: two numpy uniforms (flips), one torch normal
        (jitter); the per-pixel noise comes from the device generator keyed by one torch-drawn seed.  With the
        configuration's rotateAugmentation R > 0 a third numpy uniform per sample, after the two flip draws:
        angle = u * 2R - R (the reference's switched-off `uniform() * 4 - 2` at R = 2, scdx16p100.py:449);
        angles is None when R is 0 and no draw is made."""
        from configuration import defaultConfig
        R = defaultConfig.rotateAugmentation
        flips = np.zeros((B, 2), np.uint8)
        jit = np.zeros(B, np.float32)
        angles = np.zeros(B, np.float64) if R > 0 else None
        for b in range(B):
            flips[b, 0] = np.random.uniform() > 0.5
            flips[b, 1] = np.random.uniform() > 0.5
            if R > 0:
                angles[b] = np.random.uniform() * (2 * R) - R
            jit[b] = np.float32(1) + np.float32(JITTERSV) * torch.randn(1).numpy()[0]
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        return flips, jit, seed, angles

    def gpu_batch(self, indices, device=None):
        """A training batch augmented and target-rendered on the GPU in two launches each (scd_augment_tiles,
        scd_render_center_targets): {"xs": [(B,1,S,S)], "ys": [heat, mask, regr, inds]} on the device, the
        reference's __getitem__ stacked over `indices` (positions in the shuffled order).  With the configuration's
        rotateAugmentation > 0, scd_rotate_tiles and rotateLocs follow the augmentation and the flips.  With its
        cornerTargets on, ys = [heat, mask, regr, tl, br] from scd_render_corner_targets on the same rows, and with
        cornerEmbeddings on too, [..., tl_inds, br_inds, valid] from scd_corner_tag_inds on them (_corner_layout)."""
        from configuration import defaultConfig
        from scdhip import ops
        dev = device or self.device
        if defaultConfig.residentDataset:
            return self._resident_batch(indices, dev)
        if 0 in indices:
            shuffle(self.order)      # the reference reshuffles when index 0 is fetched (scdx16p100.py:302-305)
        ids = [self.order[i] for i in indices]
        B = len(ids)
        flips, jit, seed, angles = self._draws(B)
        tiles = torch.stack([self.samples[i] for i in ids]).to(dev)
        xs = ops.augment_tiles(tiles, torch.from_numpy(flips).to(dev), torch.from_numpy(jit).to(dev), None,
                               NOISESV, seed)
        rows = [self.flipLocs(self.bounds[i], flips[b, 0], flips[b, 1]) for b, i in enumerate(ids)]
        if angles is not None:      # rotateAugmentation > 0: the rotation comes last, as the reference wrote it
            xs = ops.rotate_tiles(xs, angles)
            rows = [self.rotateLocs(r, a) for r, a in zip(rows, angles)]
        l, n = _pack_locs(rows, trunc=True)
        l, n = torch.from_numpy(l).to(dev), torch.from_numpy(n).to(dev)
        return {"xs": [xs], "ys": _corner_layout(_render_targets(l, n), l, n)}

    # ------------------------------------------------------------------ device-resident archive
    def _buildResident(self, dev, chunk=256):
        """The whole archive on `dev`: the tiles as one (N,H,W) fp32 store in archive order, uploaded `chunk` tiles at
        a time, and the labels as CSR (rows (T,8) fp32, offsets (N+1) int64).  Raises when the tiles have more than
        one shape or when the bytes needed exceed the device's free memory; nothing is allocated then."""
        N = len(self.samples)
        shapes = {tuple(s.shape[-2:]) for s in self.samples}
        if N == 0 or len(shapes) != 1:
            raise RuntimeError("scdx16p100: residentDataset needs an archive of tiles of one shape, got %s" % (
                sorted(shapes) or "no tile"))
        H, W = shapes.pop()
        lens = [int(len(b)) for b in self.bounds]
        T = sum(lens)
        need = N * H * W * 4 + T * 8 * 4 + (N + 1) * 8
        free = int(torch.cuda.mem_get_info(dev)[0])
        if need > free:
            raise RuntimeError("scdx16p100: residentDataset needs %d bytes on %s for %d tiles of %d x %d and %d label "
                               "rows, %d bytes are free" % (need, dev, N, H, W, T, free))
        store = torch.empty(N, H, W, dtype=torch.float32, device=dev)
        for c0 in range(0, N, chunk):
            part = torch.stack(self.samples[c0:c0 + chunk]).reshape(-1, H, W)
            store[c0:c0 + len(part)].copy_(part)
        rows = torch.cat([b.reshape(-1, 8).float() for b in self.bounds]) if T else torch.zeros(0, 8)
        offsets = torch.zeros(N + 1, dtype=torch.int64)
        offsets[1:] = torch.tensor(lens, dtype=torch.int64).cumsum(0)
        self.resident = {"device": dev, "store": store, "rows": rows.to(dev), "offsets": offsets.to(dev)}
        _log("Resident Dataset: {} Tiles of {} x {} and {} Label Rows, {:.3f} GiB on {}".format(
            N, H, W, T, need / 2.0 ** 30, dev))

    def _resident_batch(self, indices, dev):
        """gpu_batch from the device-resident archive: the same draws in the same order, one upload of the batch's
        ids, flips, jitter factors and rotation coefficients, then scd_augment_tiles_indexed, scd_rotate_tiles (when
        rotateAugmentation > 0), scd_pack_locs and scd_render_center_targets (scd_render_corner_targets on the same
        device rows when cornerTargets is on, and scd_corner_tag_inds on them when cornerEmbeddings is on too).  No
        host tile or label is read and
        there is no explicit synchronise (the one upload, from pageable memory, is a blocking copy on the current
        stream, as every upload of the host path is)."""
        from scdhip import ops
        dev = torch.device(dev)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        res = getattr(self, "resident", None)
        if res is None:
            self._buildResident(dev)
            res = self.resident
        elif res["device"] != dev:
            raise RuntimeError("scdx16p100: the resident archive lives on %s, a batch for %s was asked for" % (
                res["device"], dev))
        if 0 in indices:
            shuffle(self.order)      # as gpu_batch
        ids = [self.order[i] for i in indices]
        B = len(ids)
        N = res["store"].shape[0]
        if B and not (0 <= min(ids) and max(ids) < N):
            raise IndexError("scdx16p100: tile id outside the resident archive's %d tiles" % N)
        flips, jit, seed, angles = self._draws(B)
        parts = [np.asarray(ids, np.int32), jit, flips.reshape(-1)]
        if angles is not None:      # the 8-byte values first: every view below stays aligned
            parts = [cs.numpy().reshape(-1) for cs in (ops.rotate_tiles_cs(angles), ops.pack_locs_cs(angles))] + parts
        buf = torch.from_numpy(np.concatenate([p.view(np.uint8) for p in parts])).to(dev)
        views, at = [], 0
        for p in parts:
            views.append(buf[at:at + p.nbytes])
            at += p.nbytes
        dflips, djit, dids = views[-1].view(B, 2), views[-2].view(torch.float32), views[-3].view(torch.int32)
        xs = ops.augment_tiles_indexed(res["store"], dids, dflips, djit, None, NOISESV, seed)
        cs = None
        if angles is not None:
            xs = ops.rotate_tiles(xs, None, cs=views[0].view(torch.float64).view(B, 2))
            cs = views[1].view(torch.float32).view(B, 2)
        locs, counts = ops.pack_locs(res["rows"], res["offsets"], dids, dflips, size=HEATMAPSIZE, K=MAXTAGLEN,
                                     trunc=True, cs=cs)
        return {"xs": [xs], "ys": _corner_layout(_render_targets(locs, counts), locs, counts)}

    def __getitem__(self, index):
        b = self.gpu_batch([index])
        return {"xs": [b["xs"][0][0]], "ys": [y[0] for y in b["ys"]]}


dataset = SCD


def family(ratio, percent):
    """The names of plugin module `scdx{ratio}p{percent}`: this module's, with the three constants, the SCD class and
    splitOrder bound to (ARGUMENTRATIO, PARTITION, TRAINSUBSET) = (ratio, percent / 100, 'train{ratio}p{percent}')."""
    if ratio not in (1, 4, 8, 12, 16) or percent not in (5, 10, 25, 50, 100):
        raise ValueError("no reference plugin scdx%sp%s" % (ratio, percent))
    partition, subset = percent / 100.0, "train%dp%d" % (ratio, percent)
    consts = {"ARGUMENTRATIO": ratio, "PARTITION": partition, "TRAINSUBSET": subset}
    cls = type("SCD", (SCD,), dict(consts, __module__="trainer.dataset.scdx%dp%d" % (ratio, percent)))

    def split(count, dataSplit=None):
        return splitOrder(count, dataSplit, ratio=ratio, partition=partition, subset=subset)
    split.__doc__ = splitOrder.__doc__
    names = {name: globals()[name] for name in FAMILY_NAMES}
    names.update(consts, SCD=cls, dataset=cls, splitOrder=split,
                 __all__=["SCD", "dataset", "writeArchive", "readArchive", "splitOrder"])
    return names
