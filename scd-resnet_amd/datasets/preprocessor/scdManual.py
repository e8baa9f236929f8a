"""Preprocess profile `datasets.preprocessor.scdManual` (datasets/preprocessor/scdManual.py of the reference): whole
slide RGB images plus the labeller's `;`-separated txt files -> a `.d` archive of REPEATGEN randomly rotated
copies per slide, cut x-major into destinationSize^2 tiles with per-tile `locs` rows
[ctx, cty, offx, offy, majx, majy, minl, halo] (heatmap units, 1/4 pixel).

The pixels run on the GPU: per slide the RGB image is uploaded once, scd_slide_rotate_clips (ops.slide_rotate_clips)
renders the tiles of all 16 rotations in one call -- grayscale, the margins' reflect padding, the rotation's own
reflect padding, torchvision's bilinear rotate and the tiling, without materialising a padded or rotated slide --
and the result is copied back and appended to the zip.  The reference pads and rotates the full slide on the CPU 16
times.  There is no CPU path: without a GPU generateArchieve raises.  The rotate is torchvision's tensor path
restated (see ops.slide_rotate_clips); only ResampleMode.Bilinear with PaddingMode.MirrorPadding exists here.

The label maths stays on the host, in torch float32 and in the reference's operation order (decode :58-106, the
8-fold box replication :145-155, the margin shift :157-159, rotateCoordinates :236-274, the tile assignment
:191-199).  Quirks of the reference that are reproduced:
  * REPEATGEN = 16 copies per slide;
  * one numpy.random.uniform() * 30 - 15 draw per (annotated image, repeat), in the reference's order, so
    numpy.random.seed(42) (which the reference's module sets at import) reproduces its angles;
  * an image without a txt file is skipped before any draw (and, here, before it is read);
  * the labels rotate about (width // 8, height // 8) of the UNPADDED slide, not about the padded frame's centre;
  * the replication constants `height // 2 - y - 2`, `width // 2 - x - 2` are kept exactly (a reflection about the
    slide's far edge in heatmap units would be (height - 1) / 2 - y ...);
  * the tile id (the reference's generalId) starts at 1 per image and runs on across the repeats;
  * an object whose centre is at distance 0 from the rotation centre becomes NaN (0 / 0), as there.
Deliberate deviations:
  * the output goes into the zip that is passed in, in the layout trainer.dataset.scdx16p100.readArchive /
    writeArchive define; the reference writes loose files under /hy-tmp/temp/confocalCenter and leaves the zip empty;
  * names are "<image>.<repeat>.<id>" without the ".npy" suffix the reference puts into dataset.json (its own
    reader would look for x.npy.npy);
  * object-count.json is {"count": {name: n}}, as writeArchive writes it (the reference: {"<image>.<id>": n});
  * locs are float32 (n, 8), (0, 8) when empty (the reference: float64, shape (0,) when empty);
  * settings["verbal"] (-v) is accepted and ignored;
  * a padded slide that is no multiple of destinationSize raises, before any draw for that slide (the reference
    logs and writes short tiles).
"""
import io
import json
import math
import os

import numpy
import torch

REPEATGEN = 16


def _image(path):
    from PIL import Image
    return numpy.array(Image.open(path))


def grayscale(path) -> numpy.ndarray:
    """The reference's host grayscale (:46-56): (H, W) float64 0.30 R + 0.59 G + 0.11 B.  The archive's pixels come
    from the same expression evaluated on the GPU."""
    red, green, blue = numpy.moveaxis(_image(path)[:, :, :3], 2, 0)
    return 0.30 * red + 0.59 * green + 0.11 * blue


def decode(path, imageName, width, height, iouThreshold=0.7):
    """The labeller's txt (head.x; head.y; tail.x; tail.y; minor axis length; halo radius per line, slide pixels)
    -> object rows [int cx, int cy, ox, oy, majx, majy, minl, halo] in heatmap units, or None without a txt file
    (:58-106; width, height and iouThreshold are unused there too)."""
    txtPath = os.path.join(path, os.path.splitext(imageName)[0] + ".txt")
    if not os.path.exists(txtPath):
        return None
    with open(txtPath) as annotation:
        return decodeLines(annotation.readlines())


def decodeLines(lines):
    """One object row per annotation line of six `;`-separated numbers; shorter lines are skipped.  Python floats
    (float64), as in the reference: the centre is the midpoint of head and tail, split into its heatmap cell
    (floor of a quarter) and the remainder in slide pixels; the major axis is an eighth of tail - head."""
    rows = []
    for line in lines:
        if len(line) <= 5:
            continue
        hx, hy, tx, ty, minor, halo = [float(field) for field in line.split(";")][:6]
        row = []
        for mid in ((hx + tx) / 2, (hy + ty) / 2):
            cell = mid // 4
            row.append((cell, mid - cell * 4))
        (cx, ox), (cy, oy) = row
        rows.append([cx, cy, ox, oy, (tx - hx) / 8, (ty - hy) / 8, minor / 8, halo / 4])
    return rows


def replicateBoxes(locations, width, height):
    """The objects followed by their eight mirror images across the slide's edges, for the reflect padding
    (:145-155; the constants are the reference's)."""
    mirrored = []
    fy, fx = height // 2 - 2, width // 2 - 2
    for b in locations:
        for x, y, sx, sy in ((b[0], -b[1], 1, -1), (b[0], fy - b[1], 1, -1), (-b[0], b[1], -1, 1),
                             (fx - b[0], b[1], -1, 1), (fx - b[0], -b[1], -1, -1), (-b[0], -b[1], -1, -1),
                             (fx - b[0], fy - b[1], -1, -1), (-b[0], fy - b[1], -1, -1)):
            mirrored.append([x, y, sx * b[2], sy * b[3], sx * b[4], sy * b[5], b[6], b[7]])
    return [list(b) for b in locations] + mirrored


def _turn(x, y, cosA, sinA):
    """The vector (x, y) turned by the angle whose cosine and sine are given, the way the reference does it in
    float32: through the vector's length m and its direction (x / m, y / m), so a zero vector gives NaN."""
    m = torch.sqrt(torch.pow(x, 2) + torch.pow(y, 2))
    s, c = y / m, x / m
    return m * (c * cosA - s * sinA), m * (s * cosA + c * sinA), m


def rotateCoordinates(locs, targetSizeXH, targetSizeYH, angle):
    """(n, 8) float32 rows turned clockwise by `angle` degrees, in place: the centres about
    (targetSizeXH - 0.5, targetSizeYH - 0.5), the offsets (a zero offset stays zero) and the major axes about the
    origin (:236-274 of the reference, whose float32 results this reproduces)."""
    turn = -angle * math.pi / 180      # the reference's expression; math.radians may round differently
    cosA, sinA = math.cos(turn), math.sin(turn)
    shiftX, shiftY = 0.5 - targetSizeXH, 0.5 - targetSizeYH
    locs[:, 0] += shiftX
    locs[:, 1] += shiftY
    locs[:, 0], locs[:, 1], _ = _turn(locs[:, 0].clone(), locs[:, 1].clone(), cosA, sinA)
    locs[:, 0] -= shiftX
    locs[:, 1] -= shiftY
    ox, oy, length = _turn(locs[:, 2].clone(), locs[:, 3].clone(), cosA, sinA)
    locs[:, 2] = torch.where(length == 0, torch.zeros_like(ox), ox)
    locs[:, 3] = torch.where(length == 0, torch.zeros_like(oy), oy)
    locs[:, 4], locs[:, 5], _ = _turn(locs[:, 4].clone(), locs[:, 5].clone(), cosA, sinA)
    return locs


def tileLocs(locations, width, height, margin, size, angle):
    """One repeat's labels: decode()'s rows of a width x height slide -> the (n, 8) float32 rows of every
    size x size tile of the margin-padded slide rotated by `angle`, x-major (:145-199)."""
    locations = replicateBoxes(locations, width, height)
    for row in locations:
        row[0] += margin[0] // 4
        row[1] += margin[1] // 4
    if len(locations) > 0:
        locs = rotateCoordinates(torch.tensor(locations), width // 8, height // 8, angle)
        locations = locs.double().tolist()
    padWidth, padHeight = width + margin[0] + margin[2], height + margin[1] + margin[3]
    tiles = []
    for x in range(int(padWidth / size)):
        for y in range(int(padHeight / size)):
            bs = [[b[0] - x * size // 4, b[1] - y * size // 4] + b[2:8] for b in locations
                  if x * size <= b[0] * 4 + b[2] < (x + 1) * size and y * size <= b[1] * 4 + b[3] < (y + 1) * size]
            tiles.append(numpy.array(bs, numpy.float32).reshape(-1, 8))
    return tiles


def _npy(arr):
    buf = io.BytesIO()
    numpy.save(buf, arr, allow_pickle=False)
    return buf.getvalue()


def generateArchieve(settings, imageFileNames, zipArchieve):
    """settings: preprocess.main's dict (inputImage, annotation, destinationSize, margin [l, t, r, b], ...);
    zipArchieve: an open, writable zipfile.ZipFile that receives the whole `.d` archive."""
    from tqdm import tqdm

    from scdhip import ops
    if not torch.cuda.is_available():
        raise RuntimeError("scdManual: the slide rotation kernel runs on MI355X only (no CPU fallback)")
    device = torch.device("cuda", torch.cuda.current_device())
    size, margin = settings["destinationSize"], settings["margin"]
    names, counts = [], {}
    progress = tqdm(imageFileNames)
    for imageFile in progress:
        progress.set_description(imageFile)
        imageName = os.path.splitext(imageFile)[0]
        locations = decode(settings["annotation"], imageFile, 0, 0, settings["iouThreshold"])
        if locations is None:
            continue
        rgb = _image(os.path.join(settings["inputImage"], imageFile))
        if rgb.ndim != 3 or rgb.shape[2] < 3 or rgb.dtype != numpy.uint8:
            raise RuntimeError("scdManual: %s is no 8-bit RGB image" % imageFile)
        height, width = rgb.shape[:2]
        if (width + margin[0] + margin[2]) % size != 0 or (height + margin[1] + margin[3]) % size != 0:
            raise RuntimeError("scdManual: %s is %d x %d, which the margins %s do not pad to a multiple of %d" % (
                imageFile, width, height, margin, size))
        angles = [numpy.random.uniform() * 30 - 15 for _ in range(REPEATGEN)]
        clips = ops.slide_rotate_clips(torch.from_numpy(numpy.ascontiguousarray(rgb)).to(device), margin, size,
                                       angles).cpu().numpy()
        tileId = 1
        for repeat in range(REPEATGEN):
            tiles = tileLocs(locations, width, height, margin, size, angles[repeat])
            for clip, bs in zip(clips[repeat], tiles):
                name = "%s.%d.%d" % (imageName, repeat, tileId)
                zipArchieve.writestr("samples/%s.npy" % name, _npy(clip))
                zipArchieve.writestr("locs/%s.npy" % name, _npy(bs))
                names.append(name)
                counts[name] = len(bs)
                tileId += 1
    zipArchieve.writestr("object-count.json", json.dumps({"count": counts}))
    zipArchieve.writestr("dataset.json", json.dumps({"names": names}))
