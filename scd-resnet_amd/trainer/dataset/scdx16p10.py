"""`.d` archive dataset plugin `scdx16p10` (datasets/scds/scdx16p10.py of the reference): all of the 16
preprocess rotations per slide, 10 % of their tiles.  The implementation is trainer/dataset/scdx16p100.py."""
from trainer.dataset.scdx16p100 import family

globals().update(family(16, 10))
