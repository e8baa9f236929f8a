"""`.d` archive dataset plugin `scdx8p100` (datasets/scds/scdx8p100.py of the reference): the first 8 of the 16
preprocess rotations per slide, 100 % of their tiles.  The implementation is trainer/dataset/scdx16p100.py."""
from trainer.dataset.scdx16p100 import family

globals().update(family(8, 100))
