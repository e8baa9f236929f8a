"""Slide cohort quantification (test.py:148-183 of the reference) on MI355X.

Every slide is tiled and run through the model as slide.py does; its detections are filtered to a validity box,
optionally de-duplicated across overlapping clips, and binned into the cohort's 150-bin histogram of the relative
halo radius Rhr = (halo - minl) / (2 minl) on the device (scd_slide_samples).  After the last slide the histogram
is read once, fitted with two Gaussians over the reference's bounds (scdhip/rhr.py) and reported with the six raw
parameters, the residual sum of squares and the DFI (share of component 1 by area: the project's own definition;
whether it is the paper's has not been checked).

CLI:  python quantify.py <architecture> <state_dict.pt | traced.pt> <image> [<image> ...] [-eval] [-fold]
                         [-radius R] [-box "x0 y0 x1 y1"] [-o report.json] [-samples]
  -eval / -fold   as slide.py: BN in eval mode / eval mode with BatchNorm folded into the conv operands
  -box            validity box x0 <= x < x1, y0 <= y < y1 in slide pixels; default: each slide's own 0 0 W H.
                  -box "0 0 3072 2056" reproduces the reference's notes (test.py:167)
  -radius R       drop a detection when a better-scored, kept detection of ANOTHER clip lies within R pixels
                  (clips overlap by 128 px, so an object in the overlap is reported once per clip that sees it).
                  Default -1: no de-duplication, as the reference.  No radius has been validated on real slides.
  -o report.json  also write the report as JSON
  -samples        also list each slide's kept samples (x, y, Rhr, score)
"""
import json
import sys

import numpy as np
import torch

COUNTERS = ("above", "valid", "kept", "binned", "unbinned")


def parse(argv):
    opt = {"eval": False, "fold": False, "radius": -1, "box": None, "out": None, "samples": False, "help": False}
    pos = []
    i = 0
    while i < len(argv):
        a = argv[i]
        if a in ("-h", "--help"):
            opt["help"] = True
        elif a in ("-eval", "-fold", "-samples"):
            opt[a[1:]] = True
        elif a in ("-radius", "-box", "-o"):
            if i + 1 >= len(argv):
                raise ValueError("%s needs a value" % a)
            i += 1
            if a == "-radius":
                opt["radius"] = int(argv[i])
            elif a == "-box":
                opt["box"] = [int(v) for v in argv[i].replace(",", " ").split()]
                if len(opt["box"]) != 4:
                    raise ValueError('-box needs four integers: "x0 y0 x1 y1"')
            else:
                opt["out"] = argv[i]
        else:
            pos.append(a)
        i += 1
    return opt, pos


def fit_report(hist):
    """The fit section of the report from the cohort histogram (host numpy)."""
    from scdhip import rhr
    if int(hist.sum()) == 0:
        return None, "skipped: no sample fell into the histogram"
    f = rhr.fit_gauss2(rhr.frequencies(hist))
    p = [float(v) for v in f.params]
    try:
        share = rhr.dfi(p)
    except ValueError:
        share = None
    return ({"params": p, "names": ["a1", "m1", "s1", "a2", "m2", "s2"], "sse": float(f.sse), "dfi": share,
             "iterations": int(f.iterations), "converged": bool(f.converged)},
            "ok" if f.converged else "not converged")


def quantify(wrapper, images, box=None, radius=-1, samples=False):
    """The report (a dict of plain Python values) for a cohort of image paths.  The histogram and the counters
    are read once, after the last slide; per-slide samples only when `samples` is set."""
    import slide
    from PIL import Image
    from scdhip import rhr
    dev = torch.device("cuda", torch.cuda.current_device())
    hist = torch.zeros(rhr.BINS, dtype=torch.int64, device=dev)
    per = torch.zeros(len(images), 5, dtype=torch.int64, device=dev)
    slides, kept = [], []
    for n, img in enumerate(images):
        rgb = np.array(Image.open(img))
        b = list(box) if box is not None else [0, 0, int(rgb.shape[1]), int(rgb.shape[0])]
        out = slide.analyseSamples(wrapper, rgb, b, radius, hist, per[n])
        slides.append({"image": img, "box": b})
        if samples:
            kept.append(out)
    per = per.cpu().numpy()
    hist = hist.cpu().numpy()
    for n, s in enumerate(slides):
        s["counters"] = {k: int(v) for k, v in zip(COUNTERS, per[n])}
        if samples:
            xy, ratio, score, _, count = kept[n]
            c = int(count.item())
            s["samples"] = [[int(p[0]), int(p[1]), float(r), float(sc)] for p, r, sc in
                            zip(xy[:c].cpu().tolist(), ratio[:c].cpu().tolist(), score[:c].cpu().tolist())]
    fit, status = fit_report(hist)
    return {"box": list(box) if box is not None else None, "radius": int(radius), "threshold": slide.THRESHOLD,
            "lo": rhr.LO, "scale": rhr.SCALE, "slides": slides,
            "counters": {k: int(v) for k, v in zip(COUNTERS, per.sum(0))},
            "histogram": [int(v) for v in hist], "fit": fit, "fit_status": status}


def _json_safe(v):
    """inf / NaN ratios (minl = 0) as strings: strict JSON has no spelling for them."""
    if isinstance(v, float) and not np.isfinite(v):
        return repr(v)
    if isinstance(v, list):
        return [_json_safe(x) for x in v]
    if isinstance(v, dict):
        return {k: _json_safe(x) for k, x in v.items()}
    return v


def print_report(rep):
    for s in rep["slides"]:
        c = s["counters"]
        print("%s\tbox %d %d %d %d\t%s" % (s["image"], *s["box"], "\t".join("%s %d" % (k, c[k]) for k in COUNTERS)))
        for x, y, r, sc in s.get("samples", []):
            print("%s\t%d\t%d\t%.6f\t%.6f" % (s["image"], x, y, r, sc))
    print("cohort\tradius %d\t%s" % (rep["radius"], "\t".join("%s %d" % (k, rep["counters"][k]) for k in COUNTERS)))
    print("histogram (Rhr from %.2f, bin width %.2f):" % (rep["lo"], 1.0 / rep["scale"]))
    h = rep["histogram"]
    for i in range(0, len(h), 25):
        print("  " + " ".join("%d" % v for v in h[i:i + 25]))
    if rep["fit"] is None:
        print("fit %s" % rep["fit_status"])
        return
    f = rep["fit"]
    print("fit %s\t%s" % (rep["fit_status"], "\t".join("%s %.9g" % (n, v) for n, v in zip(f["names"], f["params"]))))
    print("SSE %.9g" % f["sse"])
    print("DFI %s\t(a1 s1 / (a1 s1 + a2 s2): this project's definition, not checked against the paper's)" % (
        "%.6f" % f["dfi"] if f["dfi"] is not None else "undefined"))


def main(argv):
    try:
        opt, pos = parse(argv)
    except ValueError as e:
        print("quantify.py: %s" % e)
        return 2
    if opt["help"] or len(pos) < 3:
        print(__doc__)
        return 0 if opt["help"] else 2
    import slide
    wrapper = slide.load_wrapper(pos[0], pos[1], opt["eval"] or opt["fold"], opt["fold"])
    rep = quantify(wrapper, pos[2:], opt["box"], opt["radius"], opt["samples"])
    print_report(rep)
    if opt["out"]:
        with open(opt["out"], "w") as fh:
            json.dump(_json_safe(rep), fh, indent=1)
            fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
