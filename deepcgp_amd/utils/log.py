"""``Log`` and the host-only loggers of conv_gp/utils/log.py: a ``log.csv`` per run with one row per test period, and the run's flags
beside it as ``options.toml``."""
import csv
import math
import os


def ensure_dir(path):
    """conv_gp/utils/log.py:9-15."""
    os.makedirs(path, exist_ok=True)


class Logger(object):
    """A column of the log: ``title`` names it, ``__call__(model)`` returns the value (conv_gp/utils/log.py:17-27)."""

    def __call__(self, model):
        raise NotImplementedError()


class GlobalStepLogger(Logger):
    """Optimiser steps taken so far (conv_gp/utils/log.py:29-36).  The reference reads TensorFlow's global-step variable; here the driver
    keeps the count on the model, ``model.global_step``."""

    def __init__(self):
        self.title = "global_step"

    def __call__(self, model):
        return int(getattr(model, "global_step", 0))


class LearningRateLogger(Logger):
    """The current learning rate (conv_gp/utils/log.py:38-45).  ``learning_rate_op``: a callable without arguments, in the place of the
    reference's tensor."""

    def __init__(self, learning_rate_op):
        self.title = "lr"
        self.learning_rate_op = learning_rate_op

    def __call__(self, model):
        return self.learning_rate_op()


def _toml_string(s):
    out = []
    for ch in s:
        if ch == "\\" or ch == '"':
            out.append("\\" + ch)
        elif ch == "\n":
            out.append("\\n")
        elif ch == "\t":
            out.append("\\t")
        elif ch == "\r":
            out.append("\\r")
        elif ord(ch) < 0x20 or ord(ch) == 0x7f:
            out.append("\\u%04x" % ord(ch))
        else:
            out.append(ch)
    return '"' + "".join(out) + '"'


def _toml_value(v):
    if isinstance(v, bool):
        return "true" if v else "false"
    if isinstance(v, int):
        return str(v)
    if isinstance(v, float):
        if math.isnan(v):
            return "nan"
        if math.isinf(v):
            return "inf" if v > 0 else "-inf"
        r = repr(v)
        return r if any(c in r for c in ".en") else r + ".0"
    if isinstance(v, str):
        return _toml_string(v)
    raise TypeError("options.toml: no TOML form for %r (%s)" % (v, type(v).__name__))


def toml_lines(flags):
    """A flat dict of flags as TOML ``key = value`` lines, keys sorted.  TOML has no null: a flag that is None is left out (as the ``toml``
    package the reference writes with leaves it out) and named in a comment."""
    lines = []
    for key in sorted(flags):
        v = flags[key]
        if v is None:
            lines.append("# %s is not set" % key)
            continue
        name = key if key and all(c.isalnum() or c in "_-" for c in key) else _toml_string(key)
        lines.append("%s = %s" % (name, _toml_value(v)))
    return lines


class Log(object):
    """conv_gp/utils/log.py:85-136: ``<log_dir>/<run_name>/log.csv`` opened for appending (a restarted run goes on in the same file, under a
    second header line), one ``Entry, <titles...>`` row per ``write_entry``."""

    def __init__(self, log_dir, run_name, loggers):
        self.loggers = loggers
        self.log_dir = os.path.join(log_dir, run_name)
        ensure_dir(self.log_dir)
        self.file = open(os.path.join(self.log_dir, "log.csv"), "at", newline="")
        self.csv_writer = csv.writer(self.file)
        self.headers = ["Entry"] + [l.title for l in self.loggers]
        self.csv_writer.writerow(self.headers)
        self.file.flush()
        self.entries = 0

    def _human_readable(self, entry):
        return "; ".join("{key}: {value}".format(key=key, value=value) for key, value in zip(self.headers, entry))

    def write_entry(self, model):
        entry = [self.entries] + [logger(model) for logger in self.loggers]
        self.csv_writer.writerow(entry)
        self.file.flush()
        self.entries += 1
        return self._human_readable(entry)

    def write_flags(self, flags):
        with open(os.path.join(self.log_dir, "options.toml"), "wt") as f:
            f.write("\n".join(toml_lines(vars(flags))) + "\n")

    def close(self):
        self.file.close()
