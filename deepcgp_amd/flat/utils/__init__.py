"""Flat-import shim: ``import utils`` (conv_gp/experiment.py:6) resolves to the MI355X path's loggers with ``deepcgp_amd/flat`` on sys.path
(see INTEGRATION.md)."""
from deepcgp_amd.utils import *  # noqa: F401,F403
from deepcgp_amd.utils import Log, Logger, GlobalStepLogger, LearningRateLogger, AccuracyLogger, LogLikelihoodLogger, TestLogDensityLogger, TTAAccuracyLogger, GradNormLogger, ensure_dir  # noqa: F401
