"""TorchEasyRec's embedding, model and evaluation path on libtzrec_hip.so (gfx950).  Submodules are imported by name; the
evaluation surface is also reachable from the package (resolved on first use: importing the package loads nothing)."""
_METRICS = ("BinnedAUC", "GroupedAUC", "NormalizedEntropy", "Evaluator", "evaluate")
__all__ = list(_METRICS)


def __getattr__(name):
    if name in _METRICS:
        from . import metrics

        return getattr(metrics, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
