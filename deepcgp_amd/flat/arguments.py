"""Flat-import shim: the reference's modules import each other as top-level names (``from arguments import ...`` at
conv_gp/models.py:8-11, tests/context.py:3-4 puts conv_gp/ on sys.path).  Put ``deepcgp_amd/flat`` on sys.path in its place and
those imports resolve to the MI355X path."""
from deepcgp_amd.arguments import default_parser, parse_augmentation, parse_clip_norm, parse_dilations, parse_latent_gps, parse_paddings, parse_reselect, parse_test_views, train_steps  # noqa: F401
