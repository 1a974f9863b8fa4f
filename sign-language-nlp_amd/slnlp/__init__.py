"""slnlp: the MI355X path of the sign-language gloss classifier.  The submodules are imported on demand (``slnlp.net``,
``slnlp.ops``, ...); ``slnlp.VotingEnsemble``, ``slnlp.PriorShift``, ``slnlp.OutOfFold``, ``slnlp.cross_fit``, ``slnlp.EditKNN``,
``slnlp.PhonoKNN``, ``slnlp.split_audit``, ``slnlp.fit_field_weights``, ``slnlp.duplicate_groups`` and ``slnlp.gloss_structure`` are resolved on first use, so that ``import slnlp`` stays free of torch and sklearn."""
__all__ = ["VotingEnsemble", "PriorShift", "OutOfFold", "cross_fit", "EditKNN", "PhonoKNN", "split_audit", "fit_field_weights", "duplicate_groups", "gloss_structure"]


def __getattr__(name):
    if name == "VotingEnsemble":
        from .ensemble import VotingEnsemble
        return VotingEnsemble
    if name == "PriorShift":
        from .prior_shift import PriorShift
        return PriorShift
    if name in ("OutOfFold", "cross_fit"):
        from . import out_of_fold
        return getattr(out_of_fold, name)
    if name in ("EditKNN", "PhonoKNN", "split_audit"):
        from . import edit_knn
        return getattr(edit_knn, name)
    if name == "fit_field_weights":
        from .field_weights import fit_field_weights
        return fit_field_weights
    if name == "duplicate_groups":
        from .dup_groups import duplicate_groups
        return duplicate_groups
    if name == "gloss_structure":                            # the function's module carries its name: the module is callable
        import importlib
        return importlib.import_module(".gloss_structure", __name__)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
