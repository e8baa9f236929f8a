"""`.d` archive dataset plugin `scdx16p50` (datasets/scds/scdx16p50.py of the reference): all of the 16
preprocess rotations per slide, 50 % of their tiles.  The implementation is trainer/dataset/scdx16p100.py."""
from trainer.dataset.scdx16p100 import family

globals().update(family(16, 50))
