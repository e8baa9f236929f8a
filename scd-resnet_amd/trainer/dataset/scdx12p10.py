"""`.d` archive dataset plugin `scdx12p10` (datasets/scds/scdx12p10.py of the reference): the first 12 of the 16
preprocess rotations per slide, 10 % of their tiles.  The implementation is trainer/dataset/scdx16p100.py."""
from trainer.dataset.scdx16p100 import family

globals().update(family(12, 10))
