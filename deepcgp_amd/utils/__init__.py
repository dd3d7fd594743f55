"""The reference's ``utils`` package as its driver uses it (conv_gp/experiment.py:113-126): ``Log`` and the loggers of conv_gp/utils/log.py.  The
TensorBoard tasks (conv_gp/utils/tensorboard.py) have no counterpart -- there is no TensorFlow on this path; their one number that is worth a
column, the training log likelihood, is ``LogLikelihoodLogger``."""
from .log import Log, Logger, GlobalStepLogger, LearningRateLogger, ensure_dir, toml_lines  # noqa: F401
from ..models import AccuracyLogger, GradNormLogger, LogLikelihoodLogger, TestLogDensityLogger, TTAAccuracyLogger  # noqa: F401
