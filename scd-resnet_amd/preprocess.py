"""Build a `.d` archive from whole-slide images (preprocess.py of the reference; the command line is unchanged).

    python preprocess.py out.d -i slides/ -a annotations/ -m "l t r b" -p datasets.preprocessor.scdManual

Images are taken in the order of the leading integer of their file names.  The profile module (-p) provides
generateArchieve(settings, imageFileNames, zipArchieve) and fills the zip; datasets.preprocessor.scdManual renders
the rotated tiles on the GPU (scd_slide_rotate_clips).  The archive is what trainer.dataset.scdx{N}p{M} read.
"""
import argparse
import importlib
import os
import pprint
import re
import zipfile


def parseArguments(argv=None):
    parser = argparse.ArgumentParser(
        description="Cut annotated whole-slide images into rotated training tiles and pack them, with the decoded "
                    "object rows of every tile, into one `.d` archive.")
    parser.add_argument("outputZipPath", type=str, help="the `.d` archive (a zip) to write")
    parser.add_argument("-i", dest="inputImage", type=str, help="folder of slide images, named <integer>...")
    parser.add_argument("-a", dest="annotation", type=str, help="folder of the labeller's <image name>.txt files")
    parser.add_argument("-s", dest="destinationSize", default=512, type=int, help="tile edge in pixels")
    parser.add_argument("-t", dest="iouThreshold", default=0.7, type=float,
                        help="IoU threshold of the Gaussian radius rule (handed to the profile)")
    parser.add_argument("-v", dest="verbal", const=True, default=False, action="store_const",
                        help="kept for the reference's command line; has no effect")
    parser.add_argument("-m", dest="margin", default="0 0 0 0", type=str,
                        help="reflected border added to every slide: 'left top right bottom' in pixels")
    parser.add_argument("-p", dest="profile", type=str,
                        help="module that builds the archive: generateArchieve(settings, imageFileNames, zipArchieve)")
    return parser.parse_args(argv)


def settingsOf(args):
    """The settings dict a profile module receives (the reference's keys)."""
    settings = {key: getattr(args, key) for key in ("inputImage", "annotation", "destinationSize", "iouThreshold",
                                                    "profile")}
    settings["outputPath"] = args.outputZipPath
    settings["margin"] = [int(m) for m in args.margin.split(" ")]
    settings["verbal"] = bool(args.verbal)
    return settings


def leadingNumber(fileName):
    return int(re.match(r"\d+", fileName).group())


def main(args):
    from logger import Logger
    settings = settingsOf(args)
    Logger.info("preprocess.py: building %s with profile %s" % (settings["outputPath"], settings["profile"]))
    pprint.pprint(settings, indent=4)
    imageFileNames = sorted(os.listdir(settings["inputImage"]), key=leadingNumber)
    profile = importlib.import_module(settings["profile"])
    with zipfile.ZipFile(settings["outputPath"], "w", zipfile.ZIP_DEFLATED) as archive:
        profile.generateArchieve(settings, imageFileNames, archive)
    Logger.info("preprocess.py: wrote %s" % settings["outputPath"])
    return args


if __name__ == "__main__":
    main(parseArguments())
