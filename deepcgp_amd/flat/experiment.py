"""Flat-import shim: ``from experiment import Experiment`` (conv_gp/mnist.py:11) resolves to the MI355X driver with ``deepcgp_amd/flat`` on
sys.path."""
from deepcgp_amd.experiment import Experiment, ArrayExperiment, NpzExperiment, standardise, read_args, main  # noqa: F401
