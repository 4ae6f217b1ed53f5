"""MI355X-native mix-and-separate train step (package
``audio-visual-sepatation-in-visual-agnostic-situtation_amd``; ``import avsep_amd`` is an alias).

Layout: ``csrc/`` HIP kernels + C ABI (include/avsep.h) -> ``lib.py`` ctypes binding ->
``kernels.py`` tensor wrappers -> ``models/`` (ModelBuilder / activate surface of the reference's
models/__init__.py) and ``net_wrapper.py`` (NetWrapper / train_step surface of main.py).
"""
from . import lib, kernels, arguments, synth, resample  # noqa: F401
from . import models, net_wrapper, dp, evaluate, bss_eval, sopp, inference, checkpoint, dataset, train  # noqa: F401
from .models import ModelBuilder, activate             # noqa: F401
from .net_wrapper import NetWrapper, create_optimizer, train_step, adjust_learning_rate  # noqa: F401
from .arguments import ArgParser                       # noqa: F401

__version__ = "0.1.0"


def __getattr__(name):
    # `separate`, `localise`, `score` (and what only they use) are imported on first use, not here: `python -m avsep_amd.separate` / `.localise` / `.score` must find
    # the module un-imported (runpy refuses one that the alias has already registered under the package's real name)
    if name in ("separate", "localise", "score", "levels", "frames", "visuals", "jpeg", "png"):
        import importlib
        return importlib.import_module(__name__ + "." + name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
