"""Deformable convolution modules (models/backbones/deformable/ of the reference): see dcn_v2.py."""
from .dcn_v2 import DCN, DCNv2, dcn_v2_conv  # noqa: F401
