"""Command-line driver with the reference's config surface (/root/reference/main.py:12-143, args.py:3-53,
helper.py:307-341,415-440): one YAML file (config/config-*.yaml of the reference works unchanged) plus overrides,
then dataset -> optional balancing -> 85/15 split -> cross-validated grid search -> test metrics, writing the same
artefacts into ``workdir``:

    config.yaml                    the merged arguments                       (helper.dump_args)
    grid_search_grid_params.csv    cross product of the grid                  (helper.save_param_grid)
    grid_search_output.json        best_score / best_params / best_index      (main.tune_hyperparams)
    grid_search_results.csv        cv_results_ as a table                     (helper.save_cv_results)
    test_output.json               test_<metric> of the refitted best model   (main.test_model)
    params.pt optimizer.pt criterion.pt history.json   of the refit           (skorch Checkpoint)

    python -m slnlp.cli --config config-transformer.yaml [--grid_args '{"lr": [0.1]}'] [--max_epochs 5] ...
    python -m torch.distributed.run --nproc-per-node 8 -m slnlp.cli --config ...      # one rank per GPU

What replaces what: dask workers -> one process per GPU (``ShardedGridSearchCV``); commons-python's argument loader
-> PyYAML + argparse; torchtext / imblearn -> ``slnlp.ingest`` / ``slnlp.balance``; the torch profiler dump is not
reproduced.  ``dataset_args.synthetic: {n: ..}`` (not in the reference) generates an ASL-Phono-shaped dataset when
the corpus is not on the machine.  ``iterator_train_args: {shuffle: true, drop_last: false}`` (the reference hard-codes its
iterator arguments, helper.py:73-83, with ``shuffle`` commented out) becomes ``iterator_train__*``; in ``grid_args`` it is a grid
axis.  Configs without the key behave as before.  A top-level ``calibration: {method: temperature}`` goes to the estimator as it is
(temperature calibration on the fit's valid split, slnlp/net.py; ``{method: bias_temperature, bias_sd: 2.0}`` fits a per-class bias
beside the temperature); a list of such settings under ``grid_args`` is a grid axis.
A top-level ``error_analysis: {pairs: 20, top_k: 5}`` (both optional, these defaults) makes rank 0 write, next to test_output.json,
what ``NeuralNetClassifier.error_analysis`` finds on the test split:

    test_class_report.csv          precision / recall / f1 / support / predicted per class, then the macro row
    test_confused_pairs.csv        the most-confused (true, predicted) pairs, largest count first
    test_topk.csv                  per test sample its label and the top_k classes with their probabilities

A top-level ``confidence_intervals: {replicates: 1000, level: 0.95, seed: 0}`` (all three optional, these defaults) makes rank 0
write, next to test_output.json, what ``NeuralNetClassifier.score_interval`` finds on the test split:

    test_intervals.json            point, bootstrap mean / std and the percentile bounds of every scoring name of the run that
                                   has an interval (ECE and MCE have none), plus replicates, level, seed and rows

A top-level ``ensemble: {members: 5, voting: soft}`` (both optional, these defaults; ``voting``: soft or log; ``members`` in 2..32)
makes rank 0, after the refit, fit ``members - 1`` more estimators with the best parameters on the train data -- member i after
``torch.manual_seed(seed + i)``, without checkpoints of its own, saved under ``workdir/ensemble/member<i>/`` -- and combine them with
the refit (member 0) into a ``slnlp.ensemble.VotingEnsemble``, and write, next to test_output.json:

    test_ensemble.json             the ensemble's and every member's test scores for the run's metrics, the ensemble's
                                   ``uncertainty`` on the test split, and ``best_estimator_.compare(ensemble, test_data)``: the
                                   paired bootstrap of the single refit against the ensemble (with the ``confidence_intervals``
                                   options when that key is present, else its defaults)

A top-level ``ranking: {}`` (no options yet) makes rank 0 write, next to test_output.json, what ``NeuralNetClassifier.ranking``
finds on the test split:

    test_ranking.json              auc_macro, auc_weighted, ap_macro, ap_weighted and classes_scored
    test_ranking_classes.csv       class, name, support, one-vs-rest ROC AUC and average precision per class (an empty cell
                                   for a class without a positive or a negative test row)

A top-level ``conformal: {alpha: 0.1, method: aps, randomized: true, lam: 0.0, k_reg: 0, seed: 0}`` (all optional, these defaults;
``method``: lac or aps, ``lam`` > 0 makes it RAPS) goes to the estimator as it is (every fit takes its threshold on its valid
split, slnlp/net.py) and makes rank 0 write, next to test_output.json, what the refit's ``coverage`` finds on the test split:

    test_conformal.json            coverage, mean_size, median_size, empty_rate, singleton_rate, worst_class_coverage, rows,
                                   excluded, and the threshold: alpha, qhat, n, k
    test_conformal_classes.csv     class, name, support, coverage and mean set size per class (an empty cell for a class
                                   without a test row)

A top-level ``prior_shift: {max_iter: 200, tol: 1e-6, source: train}`` (all optional, these defaults) makes rank 0 wrap the refit in
a ``slnlp.PriorShift``, estimate the class priors of the test split from its UNLABELLED rows by EM on the device and write, next to
test_output.json:

    test_prior_shift.json          gain, d, reason, iterations, rows, nan_rows of the EM, and accuracy, balanced_accuracy and
                                   log_loss on the test split before and after the re-weighting
    test_prior_shift_classes.csv   class, name, source prior, estimated prior and test frequency per class

``source``: ``train`` -- the refit's mean predicted probability on the train data, what it learned as priors whatever the sampler
drew -- or ``train_labels`` -- the train labels' frequencies, with 1 added to every count.

A top-level ``selective: {score: max_prob, risks: [0.01, 0.05, 0.1], coverages: [0.5, 0.8, 0.9, 1.0]}`` (all optional, these
defaults; ``score``: max_prob, margin or neg_entropy; up to 8 levels each) makes rank 0 write, next to test_output.json, what the
refit's ``risk_coverage`` finds on the test split -- how wrong the fit is on what it answers when it may decline to answer:

    test_selective.json            rows, errors, accuracy, excluded_labels, excluded_nan, aurc, aurc_oracle, e_aurc, score,
                                   temperature, coverage_at_risk and risk_at_coverage (one entry per level; empirical, no guarantee)
    test_risk_coverage.csv         threshold, accepted, wrong, coverage and risk per distinct confidence threshold, descending

A top-level ``label_audit: {cv: 5, rank_by: normalized_margin, pairs: 20, top: 200}`` (all optional, these defaults; ``rank_by``:
normalized_margin or self_confidence) makes rank 0 cross-fit the refit's parameters on the TRAIN data (``slnlp.cross_fit``: ``cv``
further fits, each predicting the fold it did not see) and write what ``label_issues`` finds on those out-of-fold log-probs --
which train labels are probably wrong, by confident learning:

    train_label_audit.json         rows, bad_labels, nan_rows, unconfident, argmax_disagrees, issues, noise_rate, rank_by, cv,
                                   temperature, pairs (given, suggested, count: the likely label swaps) and per class support,
                                   threshold, issues, confident_other and noise
    train_label_issues.csv         row, given, suggested, self_confidence and margin of the first ``top`` issues, most suspicious first

(For the Transformer, whose decoder reads the gold label, this is a statement about its log-probs, not about the labels.)

A top-level ``attribution: {by: frame, mode: mask, width: 1, stride: 1, bins: 8, target: label}`` (all optional, these defaults;
``by``: frame, window or field; ``mode``: mask or drop; ``target``: label or pred) makes rank 0 write, next to test_output.json,
what the refit's ``attribute`` finds on the test split -- which frames of a sign, or which phonological fields, its predictions rest
on, by occlusion.  ``by: field`` builds the substitution table from the config's own ``dataset_args.fields`` and
``composition_strategy`` (``slnlp.ingest.field_substitutions``) and names the units after the fields:

    test_attribution.json          rows, variants, usable, bad_labels, nonfinite_rows, invalid, total_flips, temperature, the options,
                                   unit_names, the ranking (bin, name, mean drop: largest first) and per bin mean_drop, mean_kl,
                                   flip_rate, count, nonfinite
    test_attribution_classes.csv   class, name, bin, unit, count, nonfinite, mean_drop, mean_kl and flip_rate per (class, bin) with a
                                   usable variant

(For the Transformer, whose decoder reads the gold label, the drops are conditional on that label.)

A top-level ``train_dynamics: {top: 50}`` (optional, this default) goes to the estimator as ``train_dynamics=True``: every fit folds
its epochs' train log-probs into per-row integer counts on the device (csrc/train_dynamics.hip), and rank 0 writes what the
refit's ``train_dynamics()`` holds -- which train rows it never learned, learned and forgot, wavers on:

    train_dynamics.json            rows, rows_seen, unforgettable, never_learned_rows, forgetting_events, epochs, visits, bad_labels,
                                   nan_rows, bad_rows, overflow, top, the first ``top`` row indices of hard / ambiguous / forgotten /
                                   low_aum and per class support, confidence, variability, correctness, aum, never_learned, forgetting
    train_dynamics_rows.csv        row, label, name, confidence, variability, correctness, forgetting, first_learned and aum of every
                                   train row the refit has seen, by row

(The probabilities are the training pass's -- dropout on, each visit under the weights of its own step -- and for the Transformer,
whose decoder reads the gold label, conditional on that label.  The refit's checkpoints then hold train_dynamics.npz too.)

A top-level ``baseline: {k: 5, weights: distance, tau: 1.0, normalize: true, smoothing: 1.0, radius: 2, top: 50}`` (all optional,
these defaults) fits ``slnlp.EditKNN`` -- k nearest train rows under Levenshtein distance, csrc/edit_knn.hip: the method that needs
no network -- on the train split and audits the split with ``slnlp.split_audit``; rank 0 writes

    test_baseline.json             the baseline's test_<metric> scores (the metrics of test_output.json, through the same score
                                   path), its options, the neighbour summary (nearest-distance histogram, 1-NN accuracy, flagged
                                   rows) and ``refit_vs_baseline``: ``compare`` of the refit against it on the test split
    test_split_audit.json          rows, radius, exact / near duplicates of test rows in train, the ones whose twin carries another
                                   label, the nearest-distance histogram, the per-class table, the ``top`` closest pairs and the
                                   refit's accuracy on the duplicated and on the clean rows
    test_split_audit_rows.csv      row, label, name, nearest train row, its label, its name, distance, duplicated and whether the
                                   refit is right, for every test row with a neighbour

(Rows longer than 64 frames are refused, not truncated: the baseline then raises before the grid search's results are written --
unless the key names a larger limit: ``baseline: {..., max_len: 128}``, an integer in 65..512, runs the baseline and the audit on the
multi-word search (``EditKNN(max_len=...)``, ``split_audit(..., max_len=...)``, csrc/edit_long.hip), which takes rows of up to
``max_len`` frames and refuses longer ones in the same way; ``radius`` then lies in 0..max_len and ``nearest_hist`` has max_len + 2
bins.  ``phono_baseline`` has no such key: the phonology-weighted search stays at 64 frames.)

A top-level ``phono_baseline: {k: 5, weights: distance, tau: 1.0, normalize: true, smoothing: 1.0, gap: null, radius: null, top: 50}``
(all optional, these defaults) does the same under the PHONOLOGY-WEIGHTED edit distance (``slnlp.PhonoKNN``, csrc/field_knn.hip):
substituting one frame for another costs the number of fields in which they differ, inserting or deleting one costs ``gap`` (null:
the number of fields F), and ``radius`` (null: F, one frame) is in field units.  The code table comes from the config's own
``dataset_args.fields`` and ``composition_strategy`` (``slnlp.ingest.field_codes``); rank 0 writes

    test_phono_baseline.json         as test_baseline.json, with ``refit_vs_phono`` -- and, when ``baseline`` is set too,
                                     ``baseline_vs_phono``: ``compare`` of the unit-cost baseline against this one on paired
                                     resamples of the test split, i.e. whether the field metric beats the unit metric on this data
    test_phono_split_audit.json      as test_split_audit.json in field units (the histogram has 64 F + 2 bins), with gap and fields
    test_phono_split_audit_rows.csv  as test_split_audit_rows.csv

Its sub-key ``fit_weights: {levels: [0, 1, 2, 4], sweeps: 2, scoring: neg_log_loss}`` (null or absent: nothing changes) fits
per-field integer weights first (``slnlp.fit_field_weights``: a coordinate search on the leave-one-out objective of the train split,
on the device) and builds the phono baseline and the phono split audit with them -- distances, ``gap`` and ``radius`` are then
in units of W, the sum of the weights.  Rank 0 also writes

    train_phono_weights.json         the search's report with the field NAMES of ``dataset_args.fields`` next to the weights.  Its
                                     objective is leave-one-out on the TRAIN split, which this data's repeated glosses flatter;
    test_phono_baseline.json         gains ``phono_vs_weighted``: ``compare`` of the unit-weight ``PhonoKNN`` against the weighted
                                     one on paired resamples of the TEST split -- the number to judge the weights by

A top-level ``grouped_splits: {radius: 0, metric: unit, max_len: null}`` (all optional, these defaults) makes the run's splits
LEAK-FREE: ``slnlp.duplicate_groups`` (csrc/dup_groups.hip) forms the connected components of "rows within ``radius`` edits of each
other" once, on the loaded dataset, BEFORE ``balance_dataset`` and the test split; the dataset carries the group ids and the test
split, the grid's folds and every fit's internal valid split keep a group on one side (a row ``balance_dataset`` over-samples keeps
its original's group).  ``metric: unit`` is ``baseline``'s distance (``max_len``: 65..512 for longer rows), ``metric: phono``
``phono_baseline``'s, from ``dataset_args.fields``, ``radius`` in field units; it takes no ``max_len``.  Rank 0 writes

    duplicate_groups.json          the options, rows, radius, max_distance, n_groups, largest, rows_in_groups, pairs, flagged,
                                   mixed_label_groups and the histogram of group sizes

Where ``baseline`` is set too, ``test_split_audit.json`` is the end-to-end proof: at a radius up to this one it reports no twin of
a test row in train.

A top-level ``gloss_structure: {metric: unit, max_len: null, top: 50}`` (all optional, these defaults) reports, before anything is
read off a model, what the glosses of the TRAIN split look like under the metric (``slnlp.gloss_structure``,
csrc/gloss_structure.hip): ``metric: unit`` is ``baseline``'s distance (``max_len``: 65..512 for longer rows), ``metric: phono``
``phono_baseline``'s, from ``dataset_args.fields``; it takes no ``max_len``.  Rank 0 writes

    train_gloss_structure.json        the options, rows, flagged, max_distance, mean_silhouette, misplaced_share, per class its name,
                                      support, silhouette and medoid row, the ``top`` closest pairs of glosses (joinable against
                                      ``test_confused_pairs.csv``) and the ``top`` misplaced rows.  With ``metric: phono`` and
                                      ``phono_baseline.fit_weights`` set: ``mean_silhouette_unit`` and ``mean_silhouette_weighted``
                                      side by side, the report itself under the fitted weights
    train_gloss_structure_rows.csv    row, label, name, a, b, silhouette, nearest gloss, its name, whether the row is its gloss's medoid
    train_gloss_distance.csv          the C x C mean distances between glosses, a header row and column of gloss names

Without the fourteen keys the workdir holds exactly the files listed above.
"""
import argparse
import copy
import csv
import datetime
import itertools
import json
import os

import numpy as np

DICT_ARGS = ("early_stopping", "gradient_clipping", "lr_scheduler", "dataset_args", "model_args", "optimizer_args",
             "criterion_args", "iterator_train_args", "grid_args", "calibration", "error_analysis", "confidence_intervals",
             "ensemble", "ranking", "conformal", "prior_shift", "selective", "label_audit", "attribution", "train_dynamics", "baseline", "phono_baseline",
             "grouped_splits", "gloss_structure")
SCALAR_ARGS = {"model": str, "optimizer": str, "criterion": str, "cv": int, "scoring": str, "verbose": int, "n_jobs": int,
               "workdir": str, "debug": lambda s: s.lower() in ("1", "true", "yes"),
               "cuda": lambda s: s.lower() in ("1", "true", "yes"), "seed": int, "lr": float, "max_epochs": int,
               "batch_size": int, "test_size": float}


def deep_merge(base, over):
    out = copy.deepcopy(base)
    for k, v in over.items():
        out[k] = deep_merge(out[k], v) if isinstance(v, dict) and isinstance(out.get(k), dict) else copy.deepcopy(v)
    return out


def load_config(path=None, overrides=None):
    import yaml
    cfg = {}
    if path:
        with open(path) as f:
            cfg = yaml.safe_load(f) or {}
    cfg = deep_merge(cfg, overrides or {})
    for k in ("model_args", "optimizer_args", "criterion_args", "grid_args", "dataset_args"):
        cfg.setdefault(k, {})
        if cfg[k] is None:
            cfg[k] = {}
    return cfg


def format_dir(workdir, **kwargs):
    """``workdir`` is a ``str.format`` template over the run's arguments plus ``{datetime:%Y-...}`` (the reference's
    config files use ``{model}`` and ``{datetime:...}``, config-transformer.yaml:4; helper.py:307-313).  No workdir ->
    the empty string."""
    if not workdir:
        return ""
    fields = dict(kwargs, datetime=datetime.datetime.now())
    return os.path.normpath(workdir.format(**fields))


def prefix_args(prefix, ensure_list=False, output=None, **kwargs):
    """Flatten nested argument dicts into skorch's double-underscore names: ``prefix_args("module", a={"b": v})`` ->
    ``{"module__a__b": v}`` (helper.py:325-341).  ``ensure_list`` wraps scalars in one-element lists, the form a
    parameter grid needs.  Iterative (explicit stack of (name, value) pairs), leaves in depth-first key order."""
    flat = {} if output is None else output
    stack = [(k if prefix is None else f"{prefix}__{k}", v) for k, v in reversed(list(kwargs.items()))]
    while stack:
        name, value = stack.pop()
        if isinstance(value, dict):
            stack.extend((f"{name}__{k}", v) for k, v in reversed(list(value.items())))
        elif ensure_list and not isinstance(value, list):
            flat[name] = [value]
        else:
            flat[name] = value
    return flat


def build_param_grid(grid_args):
    """helper.py:108-180 ``build_grid_params``: model_args -> module__*, optimizer_args -> optimizer__*,
    criterion_args -> criterion__*, iterator_train_args -> iterator_train__*, everything else (lr, ...) by its own name."""
    g = dict(grid_args or {})
    grid = {}
    grid.update(prefix_args("module", ensure_list=True, **(g.pop("model_args", None) or {})))
    grid.update(prefix_args("optimizer", ensure_list=True, **(g.pop("optimizer_args", None) or {})))
    grid.update(prefix_args("criterion", ensure_list=True, **(g.pop("criterion_args", None) or {})))
    grid.update(prefix_args("iterator_train", ensure_list=True, **(g.pop("iterator_train_args", None) or {})))
    g.pop("training_args", None)
    grid.update(prefix_args(None, ensure_list=True, **g))
    return grid


def build_net_params(args, dataset, device):
    """helper.py:41-105 ``build_net_params`` for ``slnlp.net.NeuralNetClassifier``."""
    from model.util import get_pad_idx
    model_args = {k: v for k, v in (args.get("model_args") or {}).items() if v is not None}
    crit = dict(args.get("criterion_args") or {})
    crit["ignore_index"] = get_pad_idx(dataset.vocab_y)
    p = {"module": args["model"], "criterion": args.get("criterion", "torch.nn.CrossEntropyLoss"),
         "optimizer": args.get("optimizer", "torch.optim.SGD"), "device": device,
         "scoring": args.get("scoring"), "early_stopping": args.get("early_stopping"),
         "gradient_clipping": args.get("gradient_clipping"), "lr_scheduler": args.get("lr_scheduler"),
         "checkpoint_dir": args.get("workdir") or None}
    for k in ("lr", "max_epochs", "batch_size", "verbose", "calibration", "conformal"):     # (calibration: {method: temperature}, conformal: {alpha: ...}, slnlp/net.py)
        if args.get(k) is not None:
            p[k] = args[k]
    if train_dynamics_options(args.get("train_dynamics")) is not None:
        p["train_dynamics"] = True                                              # (the key's ``top`` shapes the files, not the fit)
    if isinstance(p.get("scoring"), str):
        p["scoring"] = [p["scoring"]]
    p.update(prefix_args("module", batch_first=True, src_vocab=dataset.vocab_X, tgt_vocab=dataset.vocab_y, **model_args))
    p.update(prefix_args("optimizer", **(args.get("optimizer_args") or {})))
    p.update(prefix_args("criterion", **crit))
    p.update(prefix_args("iterator_train", **(args.get("iterator_train_args") or {})))
    return p


def load_dataset(args):
    da = dict(args.get("dataset_args") or {})
    if da.get("synthetic"):
        from .data import synthetic_dataset
        return synthetic_dataset(**da["synthetic"])
    from .ingest import build_dataset
    return build_dataset(**da)


def _jsonable(o):
    if isinstance(o, dict):
        return {str(k): _jsonable(v) for k, v in o.items()}
    if isinstance(o, (list, tuple)):
        return [_jsonable(v) for v in o]
    if isinstance(o, (np.integer,)):
        return int(o)
    if isinstance(o, (np.floating,)):
        return float(o)
    if isinstance(o, np.ndarray):
        return o.tolist()
    return o if isinstance(o, (str, int, float, bool, type(None))) else str(o)


def save_json(obj, path):
    with open(path, "w") as f:
        json.dump(_jsonable(obj), f, indent=2)


def save_param_grid(param_grid, phase, workdir):
    import pandas as pd
    cols = list(param_grid.keys())
    pd.DataFrame(list(itertools.product(*[param_grid[c] for c in cols])), columns=cols).to_csv(
        os.path.join(workdir, f"{phase}_grid_params.csv"))


def save_cv_results(cv_results, phase, workdir):
    import pandas as pd
    pd.DataFrame({k: (list(v) if not isinstance(v, list) else v) for k, v in cv_results.items()}).to_csv(
        os.path.join(workdir, f"{phase}_results.csv"))


ERROR_ANALYSIS_DEFAULTS = {"pairs": 20, "top_k": 5}
ERROR_ANALYSIS_MAX = {"pairs": 64, "top_k": 64}                                 # SLNLP_PAIRS_MAX, SLNLP_TOPK_MAX


def error_analysis_options(setting):
    """The ``error_analysis`` key with its defaults filled in -- {pairs 20, top_k 5} -- or None when the key is absent.  Anything
    but a dict over these two keys ({}: all defaults) with integer values in 1..64 raises ValueError (``top_k`` above the number of
    classes is cut to it when the files are written)."""
    if setting is None:
        return None
    if not isinstance(setting, dict):
        raise ValueError(f"error_analysis={setting!r}: expected a dict with keys among {tuple(ERROR_ANALYSIS_DEFAULTS)}")
    unknown = sorted(set(setting) - set(ERROR_ANALYSIS_DEFAULTS))
    if unknown:
        raise ValueError(f"error_analysis: unknown keys {unknown} (known: {tuple(ERROR_ANALYSIS_DEFAULTS)})")
    opts = dict(ERROR_ANALYSIS_DEFAULTS, **setting)
    for k, v in opts.items():
        if isinstance(v, bool) or not isinstance(v, int) or not 1 <= v <= ERROR_ANALYSIS_MAX[k]:
            raise ValueError(f"error_analysis: {k}={v!r}, expected an integer in 1..{ERROR_ANALYSIS_MAX[k]}")
    return opts


def save_error_analysis(est, test_data, opts, workdir):
    """``est.error_analysis(test_data, **opts)`` as three CSV files in ``workdir`` (floats written with ``repr``: they read back
    bit for bit).  A class is written as its id and, where the dataset has a label vocabulary, its name.  Returns the result."""
    names = test_data.vocab_y.itos if getattr(test_data, "vocab_y", None) is not None else None
    name = lambda c: names[int(c)] if names is not None else str(int(c))
    res = est.error_analysis(test_data, pairs=opts["pairs"], top_k=min(opts["top_k"], len(est.classes_)), matrix=False)
    rep = res["report"]
    with open(os.path.join(workdir, "test_class_report.csv"), "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["class", "name", "precision", "recall", "f1", "support", "predicted"])
        for i, c in enumerate(res["classes"]):
            w.writerow([int(c), name(c), *(repr(float(rep[k][i])) for k in ("precision", "recall", "f1")), int(rep["support"][i]),
                        int(rep["predicted"][i])])
        w.writerow(["macro", "", *(repr(res["macro"][k]) for k in ("precision", "recall", "f1")), int(rep["support"].sum()),
                    int(rep["predicted"].sum())])
    with open(os.path.join(workdir, "test_confused_pairs.csv"), "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["true", "true_name", "predicted", "predicted_name", "count"])
        for t, p, c in res["pairs"]:
            w.writerow([int(t), name(t), int(p), name(p), int(c)])
    labels, proba = res["topk"]
    k = labels.shape[1]
    with open(os.path.join(workdir, "test_topk.csv"), "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["row", "true", *(f"top{j + 1}" for j in range(k)), *(f"p{j + 1}" for j in range(k))])
        for i in range(len(labels)):
            w.writerow([i, int(test_data.y[i]), *(int(c) for c in labels[i]), *(repr(float(p)) for p in proba[i])])
    return res


RANKING_KEYS = ()                                                               # no options yet


def ranking_options(setting):
    """The ``ranking`` key -- {} -- or None when the key is absent.  Anything but a dict without keys raises ValueError."""
    if setting is None:
        return None
    if not isinstance(setting, dict):
        raise ValueError(f"ranking={setting!r}: expected a dict with keys among {RANKING_KEYS}")
    unknown = sorted(set(setting) - set(RANKING_KEYS), key=str)
    if unknown:
        raise ValueError(f"ranking: unknown keys {unknown} (known: {RANKING_KEYS})")
    return {}


def save_ranking(est, test_data, opts, workdir):
    """``est.ranking(test_data)`` as ``test_ranking.json`` (the four scores and ``classes_scored``) and
    ``test_ranking_classes.csv`` (class, name, support, auc, ap) in ``workdir``; floats are written with ``repr`` (they read back
    bit for bit), a NaN as an empty cell.  Returns the result."""
    from . import metrics
    names = test_data.vocab_y.itos if getattr(test_data, "vocab_y", None) is not None else None
    name = lambda c: names[int(c)] if names is not None else str(int(c))
    cell = lambda v: "" if v != v else repr(float(v))
    res = est.ranking(test_data, **opts)
    save_json({**{k: float(res[k]) for k in metrics.RANKING}, "classes_scored": int(res["classes_scored"])},
              os.path.join(workdir, "test_ranking.json"))
    with open(os.path.join(workdir, "test_ranking_classes.csv"), "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["class", "name", "support", "auc", "ap"])
        for i, c in enumerate(res["classes"]):
            w.writerow([int(c), name(c), int(res["support"][i]), cell(res["auc"][i]), cell(res["ap"][i])])
    return res


CONFORMAL_SCALARS = ("coverage", "mean_size", "median_size", "empty_rate", "singleton_rate", "worst_class_coverage", "rows", "excluded")


def save_conformal(est, test_data, workdir):
    """``est.coverage(test_data)`` as ``test_conformal.json`` (the report's scalars, alpha, qhat, n, k) and
    ``test_conformal_classes.csv`` (class, name, support, coverage, mean_size) in ``workdir``; floats are written with ``repr``, a
    NaN as an empty cell.  Returns the result."""
    names = test_data.vocab_y.itos if getattr(test_data, "vocab_y", None) is not None else None
    name = lambda c: names[int(c)] if names is not None else str(int(c))
    cell = lambda v: "" if v != v else repr(float(v))
    res = est.coverage(test_data)
    out = {k: (int(res[k]) if k in ("median_size", "rows", "excluded") and res[k] == res[k] else float(res[k])) for k in CONFORMAL_SCALARS}
    out.update(alpha=float(res["alpha"]), qhat=float(res["qhat"]), n=int(res["calibration_rows"]), k=int(res["k"]))
    save_json(out, os.path.join(workdir, "test_conformal.json"))
    with open(os.path.join(workdir, "test_conformal_classes.csv"), "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["class", "name", "support", "coverage", "mean_size"])
        for i, c in enumerate(res["classes"]):
            w.writerow([int(c), name(c), int(res["support"][i]), cell(res["class_coverage"][i]), cell(res["class_mean_size"][i])])
    return res


SELECTIVE_DEFAULTS = {"score": "max_prob", "risks": [0.01, 0.05, 0.1], "coverages": [0.5, 0.8, 0.9, 1.0]}
SELECTIVE_SCORES = ("max_prob", "margin", "neg_entropy")                        # slnlp/judge.py: SELECTIVE_SCORES
SELECTIVE_MAX_LEVELS = 8                                                        # SLNLP_SEL_MAX_LEVELS
SELECTIVE_SCALARS = ("rows", "errors", "accuracy", "excluded_labels", "excluded_nan", "aurc", "aurc_oracle", "e_aurc")


def selective_options(setting):
    """The ``selective`` key with its defaults filled in -- {score max_prob, risks [0.01, 0.05, 0.1], coverages [0.5, 0.8, 0.9,
    1.0]} -- or None when the key is absent.  Anything but a dict over these three keys ({}: all defaults) with ``score`` one of
    max_prob / margin / neg_entropy and ``risks`` / ``coverages`` lists of at most 8 numbers in [0, 1] raises ValueError."""
    if setting is None:
        return None
    if not isinstance(setting, dict):
        raise ValueError(f"selective={setting!r}: expected a dict with keys among {tuple(SELECTIVE_DEFAULTS)}")
    unknown = sorted(set(setting) - set(SELECTIVE_DEFAULTS), key=str)
    if unknown:
        raise ValueError(f"selective: unknown keys {unknown} (known: {tuple(SELECTIVE_DEFAULTS)})")
    opts = dict(SELECTIVE_DEFAULTS, **setting)
    if opts["score"] not in SELECTIVE_SCORES:
        raise ValueError(f"selective: score={opts['score']!r}, expected one of {SELECTIVE_SCORES}")
    for key in ("risks", "coverages"):
        v = opts[key]
        if not isinstance(v, (list, tuple)) or len(v) > SELECTIVE_MAX_LEVELS or \
                not all(isinstance(x, (int, float)) and not isinstance(x, bool) and 0.0 <= x <= 1.0 for x in v):
            raise ValueError(f"selective: {key}={v!r}, expected a list of at most {SELECTIVE_MAX_LEVELS} numbers in [0, 1]")
    return {"score": opts["score"], "risks": [float(x) for x in opts["risks"]], "coverages": [float(x) for x in opts["coverages"]]}


def save_selective(est, test_data, opts, workdir):
    """``est.risk_coverage(test_data, **opts)`` as ``test_selective.json`` (rows, errors, accuracy, the excluded rows, aurc,
    aurc_oracle, e_aurc, score, temperature and the two level tables) and ``test_risk_coverage.csv`` (threshold, accepted, wrong,
    coverage, risk per distinct threshold, descending) in ``workdir``; floats are written with ``repr`` (they read back bit for
    bit).  Returns the result."""
    res = est.risk_coverage(test_data, **opts)
    out = {k: (int(res[k]) if k in ("rows", "errors", "excluded_labels", "excluded_nan") else float(res[k])) for k in SELECTIVE_SCALARS}
    out.update(score=res["score"], temperature=float(res["temperature"]), coverage_at_risk=res["coverage_at_risk"],
               risk_at_coverage=res["risk_at_coverage"])
    save_json(out, os.path.join(workdir, "test_selective.json"))
    curve = res["curve"]
    with open(os.path.join(workdir, "test_risk_coverage.csv"), "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["threshold", "accepted", "wrong", "coverage", "risk"])
        for i in range(len(curve["threshold"])):
            w.writerow([repr(float(curve["threshold"][i])), int(curve["accepted"][i]), int(curve["wrong"][i]),
                        repr(float(curve["coverage"][i])), repr(float(curve["risk"][i]))])
    return res


def attribution_options(setting):
    """The ``attribution`` key with its defaults filled in -- {by frame, mode mask, width 1, stride 1, bins 8, target label} -- or
    None when the key is absent.  Anything but a dict over these six keys ({}: all defaults) with ``by`` frame / window / field,
    ``mode`` mask / drop, ``width`` and ``stride`` integers >= 1 (``by: frame``: width 1), ``bins`` an integer in 1..64 and
    ``target`` label / pred raises ValueError (the estimator's own check: slnlp/judge.py)."""
    if setting is None:
        return None
    if not isinstance(setting, dict):
        raise ValueError(f"attribution={setting!r}: expected a dict with keys among ('by', 'mode', 'width', 'stride', 'bins', 'target')")
    from .judge import attribution_options as checked
    return checked(setting)


def save_attribution(est, test_data, opts, dataset_args, workdir):
    """``est.attribute(test_data, **opts)`` as ``test_attribution.json`` (the counts, the options, the ranking and the per-bin table)
    and ``test_attribution_classes.csv`` (class, name, bin, unit, count, nonfinite, mean_drop, mean_kl, flip_rate per (class, bin)
    with a usable variant) in ``workdir``; floats are written with ``repr``, a NaN as null / an empty cell.  ``by: field`` builds
    the substitution table from ``dataset_args``' ``fields`` and ``composition_strategy``.  Returns the result."""
    names = test_data.vocab_y.itos if getattr(test_data, "vocab_y", None) is not None else None
    name = lambda c: names[int(c)] if names is not None else str(int(c))
    extra = {}
    if opts["by"] == "field":
        from .ingest import field_substitutions
        fields = list((dataset_args or {}).get("fields") or [])
        if not fields or getattr(test_data, "vocab_X", None) is None or not hasattr(test_data.vocab_X, "itos"):
            raise ValueError("attribution: by='field' needs dataset_args.fields and a dataset built from them (its vocabulary names the tokens)")
        extra = {"substitutions": field_substitutions(test_data.vocab_X, fields, (dataset_args or {}).get("composition_strategy", "as_words")),
                 "unit_names": fields}
    res = est.attribute(test_data, **opts, **extra)
    num = lambda v: None if v != v else float(v)
    cell = lambda v: "" if v != v else repr(float(v))
    pb, pc = res["per_bin"], res["per_class"]
    out = {k: int(res[k]) for k in ("rows", "variants", "usable", "bad_labels", "nonfinite_rows", "invalid", "total_flips")}
    out.update(temperature=float(res["temperature"]), options=dict(opts), unit_names=list(res["unit_names"]),
               ranking=[[int(b), n, num(d)] for b, n, d in res["ranking"]],
               per_bin=[{"bin": b, "unit": res["unit_names"][b], "count": int(pb["count"][b]), "nonfinite": int(pb["nonfinite"][b]),
                         "mean_drop": num(pb["mean_drop"][b]), "mean_kl": num(pb["mean_kl"][b]), "flip_rate": num(pb["flip_rate"][b])}
                        for b in range(len(res["unit_names"]))])
    save_json(out, os.path.join(workdir, "test_attribution.json"))
    with open(os.path.join(workdir, "test_attribution_classes.csv"), "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["class", "name", "bin", "unit", "count", "nonfinite", "mean_drop", "mean_kl", "flip_rate"])
        for i, c in enumerate(res["classes"]):
            for b in range(len(res["unit_names"])):
                if pc["count"][i, b] + pc["nonfinite"][i, b] > 0:
                    w.writerow([int(c), name(c), b, res["unit_names"][b], int(pc["count"][i, b]), int(pc["nonfinite"][i, b]),
                                cell(pc["mean_drop"][i, b]), cell(pc["mean_kl"][i, b]), cell(pc["flip_rate"][i, b])])
    return res


LABEL_AUDIT_DEFAULTS = {"cv": 5, "rank_by": "normalized_margin", "pairs": 20, "top": 200}
LABEL_AUDIT_RANKINGS = ("normalized_margin", "self_confidence")                 # slnlp/metrics.py: LABEL_RANKINGS
LABEL_AUDIT_MAX_CV, LABEL_AUDIT_MAX_PAIRS = 32, 64                              # SLNLP_ENSEMBLE_MAX_MEMBERS, SLNLP_PAIRS_MAX


def label_audit_options(setting):
    """The ``label_audit`` key with its defaults filled in -- {cv 5, rank_by normalized_margin, pairs 20, top 200} -- or None when the
    key is absent.  Anything but a dict over these four keys ({}: all defaults) with ``cv`` an integer in 2..32, ``rank_by``
    normalized_margin or self_confidence, ``pairs`` an integer in 1..64 and ``top`` an integer >= 0 raises ValueError."""
    if setting is None:
        return None
    if not isinstance(setting, dict):
        raise ValueError(f"label_audit={setting!r}: expected a dict with keys among {tuple(LABEL_AUDIT_DEFAULTS)}")
    unknown = sorted(set(setting) - set(LABEL_AUDIT_DEFAULTS), key=str)
    if unknown:
        raise ValueError(f"label_audit: unknown keys {unknown} (known: {tuple(LABEL_AUDIT_DEFAULTS)})")
    opts = dict(LABEL_AUDIT_DEFAULTS, **setting)
    whole = lambda v, lo, hi: isinstance(v, int) and not isinstance(v, bool) and lo <= v <= hi
    if not whole(opts["cv"], 2, LABEL_AUDIT_MAX_CV):
        raise ValueError(f"label_audit: cv={opts['cv']!r}, expected an integer in 2..{LABEL_AUDIT_MAX_CV}")
    if opts["rank_by"] not in LABEL_AUDIT_RANKINGS:
        raise ValueError(f"label_audit: rank_by={opts['rank_by']!r}, expected one of {LABEL_AUDIT_RANKINGS}")
    if not whole(opts["pairs"], 1, LABEL_AUDIT_MAX_PAIRS):
        raise ValueError(f"label_audit: pairs={opts['pairs']!r}, expected an integer in 1..{LABEL_AUDIT_MAX_PAIRS}")
    if not whole(opts["top"], 0, 2 ** 31 - 1):
        raise ValueError(f"label_audit: top={opts['top']!r}, expected an integer >= 0")
    return opts


def save_label_audit(gs, factory, train_data, opts, seed, workdir):
    """``slnlp.cross_fit`` of ``gs.best_params_`` on ``train_data`` (``opts["cv"]`` fits, fold f after ``torch.manual_seed(seed + f)``,
    ``checkpoint_dir=None``) and its ``label_issues`` as ``train_label_audit.json`` (the scalars, the pairs and the per-class table)
    and ``train_label_issues.csv`` (row, given, suggested, self_confidence, margin of the first ``opts["top"]`` issues) in
    ``workdir``; floats are written with ``repr``.  Returns (the ``OutOfFold``, the result)."""
    from .out_of_fold import cross_fit
    net = factory().set_params(**gs.best_params_).set_params(checkpoint_dir=None)
    oof = cross_fit(net, train_data, cv=opts["cv"], seed=seed)
    res = oof.label_issues(train_data, rank_by=opts["rank_by"], pairs=opts["pairs"])
    issues, per = res["issues"], res["per_class"]
    cell = lambda v: None if v != v else float(v)            # NaN: a class without rows
    out = {k: int(res[k]) for k in ("rows", "bad_labels", "nan_rows", "unconfident", "argmax_disagrees")}
    out.update(issues=int(len(issues["row"])), noise_rate=cell(res["noise_rate"]), rank_by=res["rank_by"], cv=opts["cv"],
               temperature=float(res["temperature"]), pairs=[[int(g), int(c), int(n)] for g, c, n in res["pairs"]],
               per_class=[{"class": int(c), "support": int(per["support"][i]), "threshold": cell(per["threshold"][i]),
                           "issues": int(per["issues"][i]), "confident_other": int(per["confident_other"][i]), "noise": cell(per["noise"][i])}
                          for i, c in enumerate(res["classes"])])
    save_json(out, os.path.join(workdir, "train_label_audit.json"))
    with open(os.path.join(workdir, "train_label_issues.csv"), "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["row", "given", "suggested", "self_confidence", "margin"])
        for i in range(min(opts["top"], len(issues["row"]))):
            w.writerow([int(issues["row"][i]), int(issues["given"][i]), int(issues["suggested"][i]),
                        repr(float(issues["self_confidence"][i])), repr(float(issues["margin"][i]))])
    return oof, res


TRAIN_DYNAMICS_DEFAULTS = {"top": 50}


def train_dynamics_options(setting):
    """The ``train_dynamics`` key with its default filled in -- {top 50} -- or None when the key is absent.  Anything but a dict over
    this one key ({}: the default) with ``top`` an integer >= 0 raises ValueError."""
    if setting is None:
        return None
    if not isinstance(setting, dict):
        raise ValueError(f"train_dynamics={setting!r}: expected a dict with keys among {tuple(TRAIN_DYNAMICS_DEFAULTS)}")
    unknown = sorted(set(setting) - set(TRAIN_DYNAMICS_DEFAULTS), key=str)
    if unknown:
        raise ValueError(f"train_dynamics: unknown keys {unknown} (known: {tuple(TRAIN_DYNAMICS_DEFAULTS)})")
    opts = dict(TRAIN_DYNAMICS_DEFAULTS, **setting)
    if isinstance(opts["top"], bool) or not isinstance(opts["top"], int) or not 0 <= opts["top"] <= 2 ** 31 - 1:
        raise ValueError(f"train_dynamics: top={opts['top']!r}, expected an integer >= 0")
    return opts


def save_train_dynamics(est, train_data, opts, workdir):
    """The refit's ``train_dynamics(top=opts["top"], per_row=True)`` as ``train_dynamics.json`` (the totals, the ranked lists' row
    indices and the per-class table) and ``train_dynamics_rows.csv`` (row, label, name, confidence, variability, correctness,
    forgetting, first_learned, aum: one line per train row the fit has seen, by row) in ``workdir``; floats are written with
    ``repr``.  Returns the result."""
    res = est.train_dynamics(top=opts["top"], per_row=True)
    names = train_data.vocab_y.itos if getattr(train_data, "vocab_y", None) is not None else None
    name = lambda c: names[int(c)] if names is not None else str(int(c))
    cell = lambda v: None if v != v else float(v)            # NaN: a class without a seen row
    per = res["per_class"]
    out = {k: int(res[k]) for k in ("rows", "rows_seen", "unforgettable", "never_learned_rows", "forgetting_events", "epochs", "visits",
                                    "bad_labels", "nan_rows", "bad_rows")}
    out.update(overflow=bool(res["overflow"]), top=opts["top"],
               **{k: [int(r) for r in res[k]["row"]] for k in ("hard", "ambiguous", "forgotten", "low_aum")},
               per_class=[{"class": int(c), "name": name(c), "support": int(per["support"][i]),
                           **{k: cell(per[k][i]) for k in ("confidence", "variability", "correctness", "aum")},
                           "never_learned": int(per["never_learned"][i]), "forgetting": int(per["forgetting"][i])}
                          for i, c in enumerate(per["label"])])
    save_json(out, os.path.join(workdir, "train_dynamics.json"))
    rows = res["per_row"]
    with open(os.path.join(workdir, "train_dynamics_rows.csv"), "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["row", "label", "name", "confidence", "variability", "correctness", "forgetting", "first_learned", "aum"])
        for i in np.argsort(rows["row"], kind="stable"):
            if rows["visits"][i] > 0:
                w.writerow([int(rows["row"][i]), int(rows["label"][i]), name(rows["label"][i]), repr(float(rows["confidence"][i])),
                            repr(float(rows["variability"][i])), repr(float(rows["correctness"][i])), int(rows["forgetting"][i]),
                            int(rows["first_learned"][i]), repr(float(rows["aum"][i]))])
    return res


BASELINE_DEFAULTS = {"k": 5, "weights": "distance", "tau": 1.0, "normalize": True, "smoothing": 1.0, "radius": 2, "top": 50}
BASELINE_WEIGHTS = ("uniform", "distance")                                      # SLNLP_EDIT_UNIFORM / _DISTANCE
BASELINE_MAX_K, BASELINE_MAX_RADIUS = 64, 64                                    # SLNLP_EDIT_MAX_K, SLNLP_EDIT_MAX_LEN
BASELINE_LONG_MAX_LEN = 512                                                     # SLNLP_EDIT_LONG_MAX_LEN


def baseline_options(setting):
    """The ``baseline`` key with its defaults filled in -- {k 5, weights distance, tau 1.0, normalize true, smoothing 1.0, radius 2,
    top 50} -- or None when the key is absent.  Anything but a dict over these seven keys ({}: all defaults) with ``k`` an integer
    in 1..64, ``weights`` uniform or distance, ``tau`` and ``smoothing`` finite numbers > 0, ``normalize`` a bool, ``radius`` an
    integer in 0..64 and ``top`` an integer >= 0 raises ValueError.  An eighth key, ``max_len`` (an integer in 65..512: rows of up to
    that many frames, ``radius`` then in 0..max_len), is in the result only when it was given."""
    if setting is None:
        return None
    known = tuple(BASELINE_DEFAULTS) + ("max_len",)
    if not isinstance(setting, dict):
        raise ValueError(f"baseline={setting!r}: expected a dict with keys among {known}")
    unknown = sorted(set(setting) - set(known), key=str)
    if unknown:
        raise ValueError(f"baseline: unknown keys {unknown} (known: {known})")
    opts = dict(BASELINE_DEFAULTS, **setting)
    whole = lambda v, lo, hi: isinstance(v, int) and not isinstance(v, bool) and lo <= v <= hi
    max_radius = BASELINE_MAX_RADIUS
    if "max_len" in opts:
        if not whole(opts["max_len"], BASELINE_MAX_RADIUS + 1, BASELINE_LONG_MAX_LEN):
            raise ValueError(f"baseline: max_len={opts['max_len']!r}, expected an integer in {BASELINE_MAX_RADIUS + 1}..{BASELINE_LONG_MAX_LEN} "
                             "(leave the key out for rows of at most 64 frames)")
        max_radius = opts["max_len"]
    if not whole(opts["k"], 1, BASELINE_MAX_K):
        raise ValueError(f"baseline: k={opts['k']!r}, expected an integer in 1..{BASELINE_MAX_K}")
    if opts["weights"] not in BASELINE_WEIGHTS:
        raise ValueError(f"baseline: weights={opts['weights']!r}, expected one of {BASELINE_WEIGHTS}")
    for name in ("tau", "smoothing"):
        v = opts[name]
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not 0.0 < float(v) < float("inf"):
            raise ValueError(f"baseline: {name}={v!r}, expected a finite number > 0")
    if not isinstance(opts["normalize"], bool):
        raise ValueError(f"baseline: normalize={opts['normalize']!r}, expected true or false")
    if not whole(opts["radius"], 0, max_radius):
        raise ValueError(f"baseline: radius={opts['radius']!r}, expected an integer in 0..{max_radius}")
    if not whole(opts["top"], 0, 2 ** 31 - 1):
        raise ValueError(f"baseline: top={opts['top']!r}, expected an integer >= 0")
    return opts


def save_baseline(est, train_data, test_data, opts, intervals, metrics, device, workdir):
    """``slnlp.EditKNN`` fitted on ``train_data`` and scored on ``test_data`` as ``test_baseline.json``, and ``slnlp.split_audit`` of
    the split with the refit ``est`` as the judge as ``test_split_audit.json`` / ``test_split_audit_rows.csv`` in ``workdir``.
    Returns (the ``EditKNN``, the audit)."""
    from . import metrics as M
    from .edit_knn import EditKNN, split_audit
    from .net import ScoringWrapper
    max_len = opts.get("max_len")
    knn = EditKNN(k=opts["k"], weights=opts["weights"], tau=float(opts["tau"]), normalize=opts["normalize"], smoothing=float(opts["smoothing"]),
                  device=device, max_len=max_len).fit(train_data)
    scores = {f"test_{m}": float(ScoringWrapper(m, test_data.labels())(knn, test_data, test_data.y)) for m in metrics}
    dist, idx = knn.kneighbors(test_data)
    rows = np.stack([(idx >= 0).sum(1), np.zeros(len(idx), dtype=np.int64), dist[:, 0], np.zeros(len(idx), dtype=np.int64)], axis=1)
    summary = M.knn_report(rows, np.stack([dist, idx], axis=2), test_data.y, train_data.y, **({} if max_len is None else {"max_distance": max_len}))
    save_json({"options": {k: opts[k] for k in ("k", "weights", "tau", "normalize", "smoothing") + (() if max_len is None else ("max_len",))}, "train_rows": len(train_data), "scores": scores,
               "neighbours": _jsonable(summary), "refit_vs_baseline": _jsonable(est.compare(knn, test_data, **(intervals or {})))},
              os.path.join(workdir, "test_baseline.json"))
    audit = split_audit(train_data, test_data, radius=opts["radius"], top=opts["top"], judge=est, device=device, max_len=max_len)
    per = audit["per_class"]
    names = train_data.vocab_y.itos if getattr(train_data, "vocab_y", None) is not None else None
    name = lambda c: names[int(c)] if names is not None else str(int(c))
    out = {k: audit[k] for k in ("rows", "radius", "exact_duplicates", "near_duplicates", "conflicting", "conflicting_exact", "flagged_queries",
                                 "flagged_references", "rows_duplicated", "rows_clean", "accuracy", "accuracy_duplicated", "accuracy_clean")}
    cell = lambda v: None if isinstance(v, float) and v != v else v
    out = {k: cell(v) for k, v in out.items()}
    out.update(top=opts["top"], nearest_hist=[int(c) for c in audit["nearest_hist"]], pairs=[list(p) for p in audit["pairs"]],
               per_class=[{"class": int(c), "name": name(c), "support": int(per["support"][i]), "duplicated": int(per["duplicated"][i]),
                           "conflicting": int(per["conflicting"][i])} for i, c in enumerate(per["label"])])
    save_json(out, os.path.join(workdir, "test_split_audit.json"))
    right = np.asarray(est.predict(test_data)) == np.asarray(test_data.y)
    with open(os.path.join(workdir, "test_split_audit_rows.csv"), "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["row", "label", "name", "nearest", "nearest_label", "nearest_name", "distance", "duplicated", "refit_right"])
        for i in range(len(test_data)):
            if idx[i, 0] >= 0:
                yq, yr = int(test_data.y[i]), int(train_data.y[idx[i, 0]])
                w.writerow([i, yq, name(yq), int(idx[i, 0]), yr, name(yr), int(dist[i, 0]), int(bool(audit["duplicated"][i])), int(bool(right[i]))])
    return knn, audit


PHONO_BASELINE_DEFAULTS = {"k": 5, "weights": "distance", "tau": 1.0, "normalize": True, "smoothing": 1.0, "gap": None, "radius": None, "top": 50}
PHONO_MAX_FIELDS = 16                                                           # SLNLP_FIELD_MAX_FIELDS


PHONO_FIT_WEIGHTS_DEFAULTS = {"levels": [0, 1, 2, 4], "sweeps": 2, "scoring": "neg_log_loss"}
PHONO_MAX_WEIGHT = 16                                                           # SLNLP_FIELD_MAX_WEIGHT


def phono_fit_weights_options(setting):
    """The sub-key ``phono_baseline.fit_weights`` with its defaults filled in -- {levels [0, 1, 2, 4], sweeps 2, scoring
    neg_log_loss} -- or None when it is null.  Anything but a dict over these three keys raises ValueError: ``levels`` a non-empty
    list of distinct integers in 0..16, ``sweeps`` an integer in 1..64, ``scoring`` neg_log_loss or accuracy."""
    if setting is None:
        return None
    if not isinstance(setting, dict):
        raise ValueError(f"phono_baseline: fit_weights={setting!r}, expected null or a dict with keys among {tuple(PHONO_FIT_WEIGHTS_DEFAULTS)}")
    unknown = sorted(set(setting) - set(PHONO_FIT_WEIGHTS_DEFAULTS), key=str)
    if unknown:
        raise ValueError(f"phono_baseline: fit_weights: unknown keys {unknown} (known: {tuple(PHONO_FIT_WEIGHTS_DEFAULTS)})")
    opts = dict(PHONO_FIT_WEIGHTS_DEFAULTS, **setting)
    whole = lambda v, lo, hi: isinstance(v, int) and not isinstance(v, bool) and lo <= v <= hi
    lv = opts["levels"]
    if not isinstance(lv, (list, tuple)) or not lv or not all(whole(v, 0, PHONO_MAX_WEIGHT) for v in lv) or len(set(lv)) != len(lv):
        raise ValueError(f"phono_baseline: fit_weights: levels={lv!r}, expected a list of distinct integers in 0..{PHONO_MAX_WEIGHT}")
    if not whole(opts["sweeps"], 1, 64):
        raise ValueError(f"phono_baseline: fit_weights: sweeps={opts['sweeps']!r}, expected an integer in 1..64")
    if opts["scoring"] not in ("neg_log_loss", "accuracy"):
        raise ValueError(f"phono_baseline: fit_weights: scoring={opts['scoring']!r}, expected neg_log_loss or accuracy")
    opts["levels"] = list(lv)
    return opts


def phono_baseline_options(setting):
    """The ``phono_baseline`` key with its defaults filled in -- {k 5, weights distance, tau 1.0, normalize true, smoothing 1.0, gap
    null (-> F), radius null (-> F), top 50} -- or None when the key is absent.  Anything but a dict over these eight keys ({}: all
    defaults) raises ValueError: the five voting options as ``baseline``'s, ``gap`` null or an integer in 1..16, ``radius`` null or
    an integer in 0..1024 (both are held to the F of the config's fields once the table is built), ``top`` an integer >= 0."""
    if setting is None:
        return None
    if not isinstance(setting, dict):
        raise ValueError(f"phono_baseline={setting!r}: expected a dict with keys among {tuple(PHONO_BASELINE_DEFAULTS)}")
    fit_weights = phono_fit_weights_options(setting.get("fit_weights"))          # the one sub-key: present in the result only when set
    setting = {k: v for k, v in setting.items() if k != "fit_weights"}
    unknown = sorted(set(setting) - set(PHONO_BASELINE_DEFAULTS), key=str)
    if unknown:
        raise ValueError(f"phono_baseline: unknown keys {unknown} (known: {tuple(PHONO_BASELINE_DEFAULTS)})")
    opts = dict(PHONO_BASELINE_DEFAULTS, **setting)
    whole = lambda v, lo, hi: isinstance(v, int) and not isinstance(v, bool) and lo <= v <= hi
    if not whole(opts["k"], 1, BASELINE_MAX_K):
        raise ValueError(f"phono_baseline: k={opts['k']!r}, expected an integer in 1..{BASELINE_MAX_K}")
    if opts["weights"] not in BASELINE_WEIGHTS:
        raise ValueError(f"phono_baseline: weights={opts['weights']!r}, expected one of {BASELINE_WEIGHTS}")
    for name in ("tau", "smoothing"):
        v = opts[name]
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not 0.0 < float(v) < float("inf"):
            raise ValueError(f"phono_baseline: {name}={v!r}, expected a finite number > 0")
    if not isinstance(opts["normalize"], bool):
        raise ValueError(f"phono_baseline: normalize={opts['normalize']!r}, expected true or false")
    if opts["gap"] is not None and not whole(opts["gap"], 1, PHONO_MAX_FIELDS):
        raise ValueError(f"phono_baseline: gap={opts['gap']!r}, expected null (the number of fields) or an integer in 1..{PHONO_MAX_FIELDS}")
    if opts["radius"] is not None and not whole(opts["radius"], 0, BASELINE_MAX_RADIUS * PHONO_MAX_FIELDS):
        raise ValueError(f"phono_baseline: radius={opts['radius']!r}, expected null (the number of fields) or an integer in "
                         f"0..{BASELINE_MAX_RADIUS * PHONO_MAX_FIELDS}")
    if not whole(opts["top"], 0, 2 ** 31 - 1):
        raise ValueError(f"phono_baseline: top={opts['top']!r}, expected an integer >= 0")
    if fit_weights is not None:
        opts["fit_weights"] = fit_weights
    return opts


def phono_field_codes(dataset, dataset_args, what="phono_baseline"):
    """The code table of ``phono_baseline`` (or of the key ``what``) from the config's own ``dataset_args.fields`` and
    ``composition_strategy`` (``slnlp.ingest.field_codes``); ValueError without fields or without a source vocabulary that names the
    tokens"""
    from .ingest import field_codes
    fields = list((dataset_args or {}).get("fields") or [])
    if not fields or getattr(dataset, "vocab_X", None) is None or not hasattr(dataset.vocab_X, "itos"):
        raise ValueError(f"{what}: needs dataset_args.fields and a dataset built from them (its vocabulary names the tokens)")
    if len(fields) > PHONO_MAX_FIELDS:
        raise ValueError(f"{what}: {len(fields)} fields, at most {PHONO_MAX_FIELDS} are taken")
    return field_codes(dataset.vocab_X, fields, (dataset_args or {}).get("composition_strategy", "as_words"))


GROUPED_SPLITS_DEFAULTS = {"radius": 0, "metric": "unit", "max_len": None}
GROUPED_SPLITS_METRICS = ("unit", "phono")
GROUPED_SPLITS_REPORT = ("rows", "radius", "max_distance", "n_groups", "largest", "rows_in_groups", "pairs", "flagged", "mixed_label_groups")


def grouped_splits_options(setting):
    """The ``grouped_splits`` key with its defaults filled in -- {radius 0, metric unit, max_len null} -- or None when the key is
    absent.  Anything but a dict over these three keys ({}: all defaults) raises ValueError: ``metric`` "unit" (Levenshtein distance,
    as ``baseline``) or "phono" (the phonology-weighted distance of ``phono_baseline``, from ``dataset_args.fields``); ``max_len``
    null or an integer in 65..512, with the unit metric only (the phonology-weighted search stays at 64 frames); ``radius`` an
    integer in 0..64 -- 0..max_len with ``max_len``, 0..64 x 16 in field units under "phono" (held to 64 F once the fields are
    known)."""
    if setting is None:
        return None
    known = tuple(GROUPED_SPLITS_DEFAULTS)
    if not isinstance(setting, dict):
        raise ValueError(f"grouped_splits={setting!r}: expected a dict with keys among {known}")
    unknown = sorted(set(setting) - set(known), key=str)
    if unknown:
        raise ValueError(f"grouped_splits: unknown keys {unknown} (known: {known})")
    opts = dict(GROUPED_SPLITS_DEFAULTS, **setting)
    whole = lambda v, lo, hi: isinstance(v, int) and not isinstance(v, bool) and lo <= v <= hi
    if opts["metric"] not in GROUPED_SPLITS_METRICS:
        raise ValueError(f"grouped_splits: metric={opts['metric']!r}, expected one of {GROUPED_SPLITS_METRICS}")
    max_radius = BASELINE_MAX_RADIUS * (PHONO_MAX_FIELDS if opts["metric"] == "phono" else 1)
    if opts["max_len"] is not None:
        if opts["metric"] == "phono":
            raise ValueError(f"grouped_splits: max_len={opts['max_len']!r} with metric phono: the phonology-weighted search is limited to "
                             f"{BASELINE_MAX_RADIUS} frames (only the unit metric takes max_len)")
        if not whole(opts["max_len"], BASELINE_MAX_RADIUS + 1, BASELINE_LONG_MAX_LEN):
            raise ValueError(f"grouped_splits: max_len={opts['max_len']!r}, expected null or an integer in {BASELINE_MAX_RADIUS + 1}.."
                             f"{BASELINE_LONG_MAX_LEN} (null: rows of at most 64 frames)")
        max_radius = opts["max_len"]
    if not whole(opts["radius"], 0, max_radius):
        raise ValueError(f"grouped_splits: radius={opts['radius']!r}, expected an integer in 0..{max_radius}")
    return opts


def apply_grouped_splits(dataset, opts, dataset_args, device, workdir=None):
    """``dataset`` carrying the near-duplicate groups of the ``grouped_splits`` key (``slnlp.duplicate_groups``), formed once on
    the device; with ``workdir`` the report without its per-row arrays goes to ``duplicate_groups.json`` there.  Every split
    downstream -- the test split, the grid's folds, each fit's valid split -- then keeps a group on one side."""
    from .dup_groups import duplicate_groups
    metric = {}
    if opts["metric"] == "phono":
        codes = phono_field_codes(dataset, dataset_args, "grouped_splits")
        F = int(np.asarray(codes).shape[1])
        if opts["radius"] > BASELINE_MAX_RADIUS * F:
            raise ValueError(f"grouped_splits: radius={opts['radius']!r}, expected an integer in 0..{BASELINE_MAX_RADIUS * F} (64 frames of {F} "
                             "fields)")
        metric = {"field_codes": codes}
    res = duplicate_groups(dataset, opts["radius"], max_len=opts["max_len"], device=device, **metric)
    if workdir is not None:
        sizes = np.bincount(res["sizes"])
        save_json({"options": dict(opts), **{k: int(res[k]) for k in GROUPED_SPLITS_REPORT},
                   "size_hist": {str(s): int(c) for s, c in enumerate(sizes) if c}}, os.path.join(workdir, "duplicate_groups.json"))
    return dataset.with_groups(res)


GLOSS_STRUCTURE_DEFAULTS = {"metric": "unit", "max_len": None, "top": 50}


def gloss_structure_options(setting):
    """The ``gloss_structure`` key with its defaults filled in -- {metric unit, max_len null, top 50} -- or None when the key is
    absent.  Anything but a dict over these three keys ({}: all defaults) raises ValueError: ``metric`` "unit" or "phono" as in
    ``grouped_splits``; ``max_len`` null or an integer in 65..512, with the unit metric only; ``top`` an integer in 0..10000."""
    if setting is None:
        return None
    known = tuple(GLOSS_STRUCTURE_DEFAULTS)
    if not isinstance(setting, dict):
        raise ValueError(f"gloss_structure={setting!r}: expected a dict with keys among {known}")
    unknown = sorted(set(setting) - set(known), key=str)
    if unknown:
        raise ValueError(f"gloss_structure: unknown keys {unknown} (known: {known})")
    opts = dict(GLOSS_STRUCTURE_DEFAULTS, **setting)
    whole = lambda v, lo, hi: isinstance(v, int) and not isinstance(v, bool) and lo <= v <= hi
    if opts["metric"] not in GROUPED_SPLITS_METRICS:
        raise ValueError(f"gloss_structure: metric={opts['metric']!r}, expected one of {GROUPED_SPLITS_METRICS}")
    if opts["max_len"] is not None:
        if opts["metric"] == "phono":
            raise ValueError(f"gloss_structure: max_len={opts['max_len']!r} with metric phono: the phonology-weighted search is limited to "
                             f"{BASELINE_MAX_RADIUS} frames (only the unit metric takes max_len)")
        if not whole(opts["max_len"], BASELINE_MAX_RADIUS + 1, BASELINE_LONG_MAX_LEN):
            raise ValueError(f"gloss_structure: max_len={opts['max_len']!r}, expected null or an integer in {BASELINE_MAX_RADIUS + 1}.."
                             f"{BASELINE_LONG_MAX_LEN} (null: rows of at most 64 frames)")
    if not whole(opts["top"], 0, 10000):
        raise ValueError(f"gloss_structure: top={opts['top']!r}, expected an integer in 0..10000")
    return opts


def save_gloss_structure(train_data, opts, dataset_args, device, workdir, field_codes=None, field_weights=None):
    """``slnlp.gloss_structure`` of ``train_data`` under the ``gloss_structure`` key's metric as ``train_gloss_structure.json``,
    ``train_gloss_structure_rows.csv`` and ``train_gloss_distance.csv`` in ``workdir``.  ``field_codes``: the table of the phono
    metric (None: ``phono_field_codes``); ``field_weights``: the weights ``phono_baseline.fit_weights`` fitted -- the report is
    then the weighted metric's, and the mean silhouette under unit weights is recorded beside it.  Returns the report."""
    from .gloss_structure import gloss_structure
    metric = {}
    if opts["metric"] == "phono":
        codes = phono_field_codes(train_data, dataset_args, "gloss_structure") if field_codes is None else np.asarray(field_codes)
        metric = {"field_codes": codes}
    res = gloss_structure(train_data, max_len=opts["max_len"], device=device, top=opts["top"], **metric)
    out = {"options": dict(opts)}
    if metric and field_weights is not None:
        out["mean_silhouette_unit"] = res["mean_silhouette"]
        res = gloss_structure(train_data, device=device, top=opts["top"], field_weights=[int(w) for w in field_weights], **metric)
        out.update(mean_silhouette_weighted=res["mean_silhouette"], field_weights=[int(w) for w in field_weights])
    names = train_data.vocab_y.itos if getattr(train_data, "vocab_y", None) is not None else None
    name = lambda c: str(c) if names is None or c is None else names[int(c)]
    cell = lambda v: None if isinstance(v, float) and v != v else v
    out.update({k: cell(res[k]) for k in ("rows", "flagged", "max_distance", "mean_silhouette", "misplaced_share")})
    out["per_class"] = [{"class": c.item(), "name": name(c), "support": int(res["counts"][k]), "silhouette": cell(float(res["class_silhouette"][k])),
                         "medoid": int(res["medoids"][k])} for k, c in enumerate(res["classes"])]
    out["closest_pairs"] = [[a, b, name(a), name(b), d, na, nb] for a, b, d, na, nb in res["closest_pairs"]]
    out["misplaced"] = [dict(m, name=name(m["label"]), nearest_name=name(m["nearest_class"])) for m in res["misplaced"]]
    save_json(out, os.path.join(workdir, "train_gloss_structure.json"))
    medoids = set(int(m) for m in res["medoids"] if m >= 0)
    y = np.asarray(train_data.y)
    with open(os.path.join(workdir, "train_gloss_structure_rows.csv"), "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["row", "label", "name", "a", "b", "silhouette", "nearest_class", "nearest_name", "medoid"])
        for i in range(len(train_data)):
            near = res["nearest_class"][i]
            w.writerow([i, int(y[i]), name(y[i]), res["a"][i], res["b"][i], res["silhouette"][i], "" if near is None else near,
                        "" if near is None else name(near), int(i in medoids)])
    with open(os.path.join(workdir, "train_gloss_distance.csv"), "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["", *[name(c) for c in res["classes"]]])
        for k, c in enumerate(res["classes"]):
            w.writerow([name(c), *res["class_distance"][k].tolist()])
    return res


def save_phono_baseline(est, train_data, test_data, opts, dataset_args, intervals, metrics, device, workdir, unit=None, field_codes=None):
    """``slnlp.PhonoKNN`` fitted on ``train_data`` and scored on ``test_data`` as ``test_phono_baseline.json``, and
    ``slnlp.split_audit(field_codes=...)`` of the split with the refit ``est`` as the judge as ``test_phono_split_audit.json`` /
    ``test_phono_split_audit_rows.csv`` in ``workdir``.  ``field_codes``: the table (None: ``phono_field_codes``).  ``unit``: the
    fitted ``EditKNN`` of the ``baseline`` key when that is set too -- ``baseline_vs_phono`` is its ``compare`` against the field
    metric on paired resamples.  With ``opts["fit_weights"]`` the weights are fitted on ``train_data`` first
    (``train_phono_weights.json``), the baseline and the audit run under them (units of W) and ``phono_vs_weighted`` compares the
    unit-weight ``PhonoKNN`` against the weighted one.  Returns (the ``PhonoKNN``, the audit)."""
    from . import metrics as M
    from .edit_knn import PhonoKNN, split_audit
    from .net import ScoringWrapper
    codes = phono_field_codes(train_data, dataset_args) if field_codes is None else np.asarray(field_codes)
    F = int(codes.shape[1])
    fit, fweights, unit_knn = opts.get("fit_weights"), None, None
    gap = F if opts["gap"] is None else opts["gap"]
    if not 1 <= gap <= F:
        raise ValueError(f"phono_baseline: gap={gap!r}, expected null or an integer in 1..{F} (the number of fields)")
    vote = dict(k=opts["k"], weights=opts["weights"], tau=float(opts["tau"]), normalize=opts["normalize"], smoothing=float(opts["smoothing"]), device=device)
    if fit is not None:
        from .field_weights import fit_field_weights
        if opts["radius"] is not None and not 0 <= opts["radius"] <= BASELINE_MAX_RADIUS * PHONO_MAX_WEIGHT:
            raise ValueError(f"phono_baseline: radius={opts['radius']!r}, expected null or an integer in 0..{BASELINE_MAX_RADIUS * PHONO_MAX_WEIGHT}")
        report = fit_field_weights(train_data, codes, levels=fit["levels"], sweeps=fit["sweeps"], scoring=fit["scoring"], gap=opts["gap"], **vote)
        fweights = [int(v) for v in report["weights"]]
        names = list((dataset_args or {}).get("fields") or [])
        names = names if len(names) == F else [f"field{f}" for f in range(F)]
        save_json(_jsonable({**report, "fields": dict(zip(names, fweights)), "field_names": names, "options": {**fit, "gap": opts["gap"]},
                             "note": "leave-one-out on the train split: repeated glosses flatter it; judge the weights by phono_vs_weighted "
                                     "in test_phono_baseline.json"}), os.path.join(workdir, "train_phono_weights.json"))
        unit_knn = PhonoKNN(codes, gap=gap, **vote).fit(train_data)
        F_unit, F = F, sum(fweights)                             # from here on the unit is W
        gap = F if opts["gap"] is None else opts["gap"]
    radius = F if opts["radius"] is None else opts["radius"]
    if not 0 <= radius <= BASELINE_MAX_RADIUS * F:
        raise ValueError(f"phono_baseline: radius={radius!r}, expected null or an integer in 0..{BASELINE_MAX_RADIUS * F} (64 frames of {F} fields)")
    if fweights is None:
        knn = PhonoKNN(codes, gap=gap, **vote).fit(train_data)
    else:
        knn = PhonoKNN(codes, gap=gap, field_weights=fweights, **vote).fit(train_data)
    scores = {f"test_{m}": float(ScoringWrapper(m, test_data.labels())(knn, test_data, test_data.y)) for m in metrics}
    dist, idx = knn.kneighbors(test_data)
    rows = np.stack([(idx >= 0).sum(1), np.zeros(len(idx), dtype=np.int64), dist[:, 0], np.zeros(len(idx), dtype=np.int64)], axis=1)
    summary = M.knn_report(rows, np.stack([dist, idx], axis=2), test_data.y, train_data.y, max_distance=BASELINE_MAX_RADIUS * F)
    base = {"options": {**{k: opts[k] for k in ("k", "weights", "tau", "normalize", "smoothing")}, "gap": gap, "fields": F}, "train_rows": len(train_data),
            "scores": scores, "neighbours": _jsonable(summary), "refit_vs_phono": _jsonable(est.compare(knn, test_data, **(intervals or {})))}
    if unit is not None:
        base["baseline_vs_phono"] = _jsonable(unit.compare(knn, test_data, **(intervals or {})))
    if fweights is not None:
        base["options"].update(fields=F_unit, field_weights=fweights, unit=F)
        base["phono_vs_weighted"] = _jsonable(unit_knn.compare(knn, test_data, **(intervals or {})))
    save_json(base, os.path.join(workdir, "test_phono_baseline.json"))
    audit = split_audit(train_data, test_data, radius=radius, top=opts["top"], judge=est, device=device, field_codes=codes, gap=gap,
                        **({} if fweights is None else {"field_weights": fweights}))
    per = audit["per_class"]
    names = train_data.vocab_y.itos if getattr(train_data, "vocab_y", None) is not None else None
    name = lambda c: names[int(c)] if names is not None else str(int(c))
    out = {k: audit[k] for k in ("rows", "radius", "exact_duplicates", "near_duplicates", "conflicting", "conflicting_exact", "flagged_queries",
                                 "flagged_references", "rows_duplicated", "rows_clean", "accuracy", "accuracy_duplicated", "accuracy_clean")}
    cell = lambda v: None if isinstance(v, float) and v != v else v
    out = {k: cell(v) for k, v in out.items()}
    out.update(top=opts["top"], gap=gap, fields=F, nearest_hist=[int(c) for c in audit["nearest_hist"]], pairs=[list(p) for p in audit["pairs"]],
               per_class=[{"class": int(c), "name": name(c), "support": int(per["support"][i]), "duplicated": int(per["duplicated"][i]),
                           "conflicting": int(per["conflicting"][i])} for i, c in enumerate(per["label"])])
    if fweights is not None:
        out.update(fields=F_unit, field_weights=fweights, unit=F)
    save_json(out, os.path.join(workdir, "test_phono_split_audit.json"))
    right = np.asarray(est.predict(test_data)) == np.asarray(test_data.y)
    with open(os.path.join(workdir, "test_phono_split_audit_rows.csv"), "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["row", "label", "name", "nearest", "nearest_label", "nearest_name", "distance", "duplicated", "refit_right"])
        for i in range(len(test_data)):
            if idx[i, 0] >= 0:
                yq, yr = int(test_data.y[i]), int(train_data.y[idx[i, 0]])
                w.writerow([i, yq, name(yq), int(idx[i, 0]), yr, name(yr), int(dist[i, 0]), int(bool(audit["duplicated"][i])), int(bool(right[i]))])
    return knn, audit


PRIOR_SHIFT_DEFAULTS = {"max_iter": 200, "tol": 1e-6, "source": "train"}
PRIOR_SHIFT_MAX_ITER = 1024                                                     # SLNLP_PRIOR_MAX_ITER
PRIOR_SHIFT_SOURCES = ("train", "train_labels")
PRIOR_SHIFT_SCORES = ("accuracy", "balanced_accuracy", "neg_log_loss")


def prior_shift_options(setting):
    """The ``prior_shift`` key with its defaults filled in -- {max_iter 200, tol 1e-6, source train} -- or None when the key is
    absent.  Anything but a dict over these three keys ({}: all defaults) with ``max_iter`` an integer in 0..1024, ``tol`` a finite
    number >= 0 and ``source`` "train" or "train_labels" raises ValueError."""
    if setting is None:
        return None
    if not isinstance(setting, dict):
        raise ValueError(f"prior_shift={setting!r}: expected a dict with keys among {tuple(PRIOR_SHIFT_DEFAULTS)}")
    unknown = sorted(set(setting) - set(PRIOR_SHIFT_DEFAULTS), key=str)
    if unknown:
        raise ValueError(f"prior_shift: unknown keys {unknown} (known: {tuple(PRIOR_SHIFT_DEFAULTS)})")
    opts = dict(PRIOR_SHIFT_DEFAULTS, **setting)
    if isinstance(opts["tol"], str):                                            # YAML 1.1 reads ``1e-6`` (no dot) as a string
        try:
            opts["tol"] = float(opts["tol"])
        except ValueError:
            pass
    if isinstance(opts["max_iter"], bool) or not isinstance(opts["max_iter"], int) or not 0 <= opts["max_iter"] <= PRIOR_SHIFT_MAX_ITER:
        raise ValueError(f"prior_shift: max_iter={opts['max_iter']!r}, expected an integer in 0..{PRIOR_SHIFT_MAX_ITER}")
    if isinstance(opts["tol"], bool) or not isinstance(opts["tol"], (int, float)) or not 0.0 <= opts["tol"] < float("inf"):
        raise ValueError(f"prior_shift: tol={opts['tol']!r}, expected a finite number >= 0")
    if opts["source"] not in PRIOR_SHIFT_SOURCES:
        raise ValueError(f"prior_shift: source={opts['source']!r}, expected one of {PRIOR_SHIFT_SOURCES}")
    return {"max_iter": int(opts["max_iter"]), "tol": float(opts["tol"]), "source": opts["source"]}


def save_prior_shift(est, train_data, test_data, opts, workdir):
    """``PriorShift(est, source).fit(test_data)`` -- ``source`` the train data itself or its smoothed label frequencies -- as
    ``test_prior_shift.json`` (the EM's scalars and {accuracy, balanced_accuracy, log_loss} on the test split ``before`` and
    ``after``) and ``test_prior_shift_classes.csv`` (class, name, source_prior, estimated_prior, test_frequency) in ``workdir``;
    floats are written with ``repr``.  Returns (the wrapper, what it wrote)."""
    from .net import ScoringWrapper, _CachedPredictor
    from .prior_shift import PriorShift, class_frequencies
    V = len(est.classes_)
    source = train_data if opts["source"] == "train" else class_frequencies(train_data.y, V, smoothing=1.0)
    shifted = PriorShift(est, source).fit(test_data, max_iter=opts["max_iter"], tol=opts["tol"])
    labels = np.arange(V)

    def scores(e):                                                              # one forward pass per estimator
        cached = _CachedPredictor(e.predict_proba(test_data), e.classes_)
        got = {n: float(ScoringWrapper(n, labels)(cached, test_data, test_data.y)) for n in PRIOR_SHIFT_SCORES}
        return {"accuracy": got["accuracy"], "balanced_accuracy": got["balanced_accuracy"], "log_loss": -got["neg_log_loss"]}
    info = shifted.prior_shift_
    out = {"gain": float(info["gain"]), "d": float(info["d"]), "reason": info["reason"], "iterations": int(info["iterations"]),
           "rows": int(info["rows"]), "nan_rows": int(info["nan_rows"]), "source": opts["source"], "max_iter": opts["max_iter"],
           "tol": opts["tol"], "before": scores(est), "after": scores(shifted)}
    save_json(out, os.path.join(workdir, "test_prior_shift.json"))
    names = test_data.vocab_y.itos if getattr(test_data, "vocab_y", None) is not None else None
    name = lambda c: names[int(c)] if names is not None else str(int(c))
    y = np.asarray(test_data.y)
    freq = np.bincount(y[(y >= 0) & (y < V)], minlength=V) / max(1, len(y))
    with open(os.path.join(workdir, "test_prior_shift_classes.csv"), "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["class", "name", "source_prior", "estimated_prior", "test_frequency"])
        for i, c in enumerate(shifted.classes_):
            w.writerow([int(c), name(c), repr(float(shifted.source_priors_[i])), repr(float(shifted.priors_[i])), repr(float(freq[i]))])
    return shifted, out


INTERVAL_DEFAULTS = {"replicates": 1000, "level": 0.95, "seed": 0}
INTERVAL_MAX_REPLICATES = 65536                                                 # SLNLP_BOOT_MAX_REPLICATES


def confidence_interval_options(setting):
    """The ``confidence_intervals`` key with its defaults filled in -- {replicates 1000, level 0.95, seed 0} -- or None when the key
    is absent.  Anything but a dict over these three keys ({}: all defaults) with ``replicates`` an integer in 2..65536 (one
    replicate has no standard deviation, and the file holds numbers only), ``level`` a number in (0, 1) and ``seed`` an integer in
    [0, 2^64) raises ValueError."""
    if setting is None:
        return None
    if not isinstance(setting, dict):
        raise ValueError(f"confidence_intervals={setting!r}: expected a dict with keys among {tuple(INTERVAL_DEFAULTS)}")
    unknown = sorted(set(setting) - set(INTERVAL_DEFAULTS))
    if unknown:
        raise ValueError(f"confidence_intervals: unknown keys {unknown} (known: {tuple(INTERVAL_DEFAULTS)})")
    opts = dict(INTERVAL_DEFAULTS, **setting)
    whole = lambda v: isinstance(v, int) and not isinstance(v, bool)
    if not whole(opts["replicates"]) or not 2 <= opts["replicates"] <= INTERVAL_MAX_REPLICATES:
        raise ValueError(f"confidence_intervals: replicates={opts['replicates']!r}, expected an integer in 2..{INTERVAL_MAX_REPLICATES}")
    if isinstance(opts["level"], bool) or not isinstance(opts["level"], (int, float)) or not 0.0 < opts["level"] < 1.0:
        raise ValueError(f"confidence_intervals: level={opts['level']!r}, expected a number in (0, 1)")
    if not whole(opts["seed"]) or not 0 <= opts["seed"] < 2 ** 64:
        raise ValueError(f"confidence_intervals: seed={opts['seed']!r}, expected an integer in [0, 2^64)")
    return opts


def save_intervals(est, test_data, opts, names, workdir):
    """``est.score_interval(test_data, **opts)`` for the scoring names among ``names`` that have an interval, as
    ``test_intervals.json`` in ``workdir``: {replicates, level, seed, rows, intervals: {test_<name>: {point, mean, std, lower, upper,
    n_nan}}}.  One call serves one top-k, so names with different k take a call each, under the same seed; a ``top<k>_accuracy``
    whose k is not below the number of classes has no value (``test_output.json`` could not hold it either) and is left out, like the
    names without an interval.  Returns what it wrote."""
    from . import metrics
    by_k = {}                                                                   # k of the top-k column (None: not used) -> names
    for n in dict.fromkeys(names):
        found = metrics.bootstrap_metric_of(n) if isinstance(n, str) else None
        if found is not None and (found[2] is None or 1 <= found[2] < len(est.classes_)):
            by_k.setdefault(found[2], []).append(n)
    plain, ks = by_k.pop(None, []), sorted(by_k)
    groups = [g for g in [plain + (by_k[ks[0]] if ks else []), *(by_k[k] for k in ks[1:])] if g]
    out = {"replicates": opts["replicates"], "level": opts["level"], "seed": opts["seed"], "rows": len(test_data), "intervals": {}}
    for group in groups:
        res = est.score_interval(test_data, scoring=group, **opts)
        out["intervals"].update({f"test_{n}": res[n] for n in group})
    save_json(out, os.path.join(workdir, "test_intervals.json"))
    return out


ENSEMBLE_DEFAULTS = {"members": 5, "voting": "soft"}
ENSEMBLE_MAX_MEMBERS = 32                                                       # SLNLP_ENSEMBLE_MAX_MEMBERS
ENSEMBLE_VOTING = ("soft", "log")


def ensemble_options(setting):
    """The ``ensemble`` key with its defaults filled in -- {members 5, voting soft} -- or None when the key is absent.  Anything but
    a dict over these two keys ({}: all defaults) with ``members`` an integer in 2..32 (one member is the refit itself) and
    ``voting`` "soft" or "log" raises ValueError."""
    if setting is None:
        return None
    if not isinstance(setting, dict):
        raise ValueError(f"ensemble={setting!r}: expected a dict with keys among {tuple(ENSEMBLE_DEFAULTS)}")
    unknown = sorted(set(setting) - set(ENSEMBLE_DEFAULTS))
    if unknown:
        raise ValueError(f"ensemble: unknown keys {unknown} (known: {tuple(ENSEMBLE_DEFAULTS)})")
    opts = dict(ENSEMBLE_DEFAULTS, **setting)
    if isinstance(opts["members"], bool) or not isinstance(opts["members"], int) or not 2 <= opts["members"] <= ENSEMBLE_MAX_MEMBERS:
        raise ValueError(f"ensemble: members={opts['members']!r}, expected an integer in 2..{ENSEMBLE_MAX_MEMBERS}")
    if opts["voting"] not in ENSEMBLE_VOTING:
        raise ValueError(f"ensemble: voting={opts['voting']!r}, expected one of {ENSEMBLE_VOTING}")
    return opts


def save_ensemble(gs, factory, train_data, test_data, opts, intervals, names, seed, workdir):
    """The refit (member 0) and ``opts["members"] - 1`` further fits of ``gs.best_params_`` on ``train_data`` -- member i after
    ``torch.manual_seed(seed + i)``, ``checkpoint_dir=None``, saved under ``workdir/ensemble/member<i>/`` -- as a
    ``VotingEnsemble``; ``test_ensemble.json`` in ``workdir``: {members, voting, scores: {ensemble, members}, uncertainty,
    single_vs_ensemble}.  Names whose top-k is not below the number of classes have no value and are left out, as in
    ``save_intervals``.  Returns (the ensemble, what it wrote)."""
    import torch

    from . import metrics
    from .ensemble import VotingEnsemble
    members = [gs.best_estimator_]
    for i in range(1, opts["members"]):
        net = factory().set_params(**gs.best_params_).set_params(checkpoint_dir=None)
        torch.manual_seed(seed + i)
        net.fit(train_data)
        net.save_params(os.path.join(workdir, "ensemble", f"member{i}"))
        members.append(net)
    ens = VotingEnsemble(members, voting=opts["voting"])
    V = len(ens.classes_)
    names = [n for n in dict.fromkeys(names) if metrics.top_k_of(n) is None or 1 <= metrics.top_k_of(n) < V]
    scores = ens.member_scores(test_data, names)
    out = {"members": len(members), "voting": opts["voting"],
           "scores": {"ensemble": {f"test_{n}": v for n, v in scores["ensemble"].items()},
                      "members": [{f"test_{n}": v for n, v in m.items()} for m in scores["members"]]},
           "uncertainty": ens.uncertainty(test_data),
           "single_vs_ensemble": gs.best_estimator_.compare(ens, test_data, **(intervals or {}))}
    save_json(out, os.path.join(workdir, "test_ensemble.json"))
    return ens, out


def run(args):
    """main.run + tune_hyperparams + test_model.  Returns (grid search object, test metrics); rank 0 writes files."""
    import random

    import torch

    from . import grid as G
    from .balance import balance_dataset
    from .net import NeuralNetClassifier, ScoringWrapper, conformal_options

    seed = int(args.get("seed", 1))
    torch.manual_seed(seed); random.seed(seed); np.random.seed(seed)            # helper.setup_seed
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise RuntimeError("slnlp.cli: needs an MI355X -- the HIP path is the only compute path")
    torch.cuda.set_device(local)
    device = f"cuda:{local}"
    if world > 1:
        import torch.distributed as dist
        if not dist.is_initialized():
            # the only collectives are the dataset broadcast and the score all_gather, hours apart on a full grid:
            # the default 10-minute watchdog would abort ranks that wait for a slower one
            dist.init_process_group("nccl", device_id=torch.device(device), timeout=datetime.timedelta(hours=48))
    workdir = args.get("workdir") or "."
    analysis = error_analysis_options(args.get("error_analysis"))               # a bad key fails before the grid search, not after
    intervals = confidence_interval_options(args.get("confidence_intervals"))
    ensemble = ensemble_options(args.get("ensemble"))
    ranking = ranking_options(args.get("ranking"))
    conformal = conformal_options(args.get("conformal"))                         # (the estimator's own check: slnlp/net.py)
    prior_shift = prior_shift_options(args.get("prior_shift"))
    selective = selective_options(args.get("selective"))
    label_audit = label_audit_options(args.get("label_audit"))
    attribution = attribution_options(args.get("attribution"))
    dynamics = train_dynamics_options(args.get("train_dynamics"))
    baseline = baseline_options(args.get("baseline"))
    phono = phono_baseline_options(args.get("phono_baseline"))
    grouped = grouped_splits_options(args.get("grouped_splits"))
    structure = gloss_structure_options(args.get("gloss_structure"))
    if rank == 0:
        os.makedirs(workdir, exist_ok=True)
        import yaml
        with open(os.path.join(workdir, "config.yaml"), "w") as f:
            yaml.safe_dump(_jsonable(args), f)

    dataset = load_dataset(args) if rank == 0 else None
    if world > 1:
        dataset = G.broadcast_dataset(dataset, device)
    if args.get("debug"):
        dataset = dataset.truncated(int(args.get("cv", 5)) * 10)
    if grouped is not None:                                  # before the rows are over-sampled and split: a copy keeps its original's group
        dataset = apply_grouped_splits(dataset, grouped, args.get("dataset_args"), device, workdir if rank == 0 else None)
    if (args.get("dataset_args") or {}).get("balance_dataset") is True:
        dataset = balance_dataset(dataset, seed)
    test_data, train_data = dataset.split(float(args.get("test_size", 0.15)), seed)
    phono_codes = phono_field_codes(dataset, args.get("dataset_args")) if phono is not None else None      # fails before the grid search
    if structure is not None and structure["metric"] == "phono" and phono_codes is None:
        phono_codes = phono_field_codes(dataset, args.get("dataset_args"), "gloss_structure")

    net_params = build_net_params(args, dataset, device)
    factory = lambda: NeuralNetClassifier(**net_params)
    scoring = args.get("scoring") or "neg_log_loss"
    first_score = scoring[0] if isinstance(scoring, list) else scoring
    param_grid = build_param_grid(args.get("grid_args"))
    gs = G.ShardedGridSearchCV(factory, param_grid, cv=int(args.get("cv", 5)), scoring=first_score, refit=True,
                               device=device, verbose=int(args.get("verbose", 0) or 0),
                               fits_per_gpu=int(args.get("fits_per_gpu", 1)), seed=seed)
    gs.fit(train_data)
    test_output = None
    if rank == 0:
        phase = "grid_search"
        save_param_grid(param_grid, phase, workdir)
        save_json({"best_score": float(gs.best_score_), "best_params": gs.best_params_, "best_index": int(gs.best_index_),
                   "scoring": repr(ScoringWrapper(first_score, train_data.labels()))}, os.path.join(workdir, f"{phase}_output.json"))
        save_cv_results(gs.cv_results_, phase, workdir)
        metrics = scoring if isinstance(scoring, list) else [scoring]
        if "accuracy" not in metrics:
            metrics = ["accuracy", *metrics]                                    # main.test_model
        est = gs.best_estimator_
        test_output = {f"test_{m}": float(ScoringWrapper(m, test_data.labels())(est, test_data, test_data.y)) for m in metrics}
        save_json(test_output, os.path.join(workdir, "test_output.json"))
        if analysis is not None:
            save_error_analysis(est, test_data, analysis, workdir)
        if intervals is not None:
            save_intervals(est, test_data, intervals, metrics, workdir)
        if ranking is not None:
            save_ranking(est, test_data, ranking, workdir)
        if conformal is not None:
            save_conformal(est, test_data, workdir)
        if selective is not None:
            save_selective(est, test_data, selective, workdir)
        if attribution is not None:
            save_attribution(est, test_data, attribution, args.get("dataset_args"), workdir)
        if ensemble is not None:
            save_ensemble(gs, factory, train_data, test_data, ensemble, intervals, metrics, seed, workdir)
        if prior_shift is not None:
            save_prior_shift(est, train_data, test_data, prior_shift, workdir)
        if label_audit is not None:
            save_label_audit(gs, factory, train_data, label_audit, seed, workdir)
        if dynamics is not None:
            save_train_dynamics(est, train_data, dynamics, workdir)
        unit = None
        if baseline is not None:
            unit, _ = save_baseline(est, train_data, test_data, baseline, intervals, metrics, device, workdir)
        phono_knn = None
        if phono is not None:
            phono_knn, _ = save_phono_baseline(est, train_data, test_data, phono, args.get("dataset_args"), intervals, metrics, device, workdir,
                                               unit=unit, field_codes=phono_codes)
        if structure is not None:
            save_gloss_structure(train_data, structure, args.get("dataset_args"), device, workdir, field_codes=phono_codes,
                                 field_weights=getattr(phono_knn, "field_weights", None))
        # workdir/{params,optimizer,criterion}.pt + history.json are the refit's best-valid-loss checkpoint (skorch
        # Checkpoint(monitor="valid_loss_best", dirname=workdir), helper.py:211-213) and stay untouched; the weights
        # after the last epoch (not kept by the reference) go to a directory of their own
        est.save_params(os.path.join(workdir, "final"))
    if world > 1:
        _wait_for_rank0(rank, world)
    return gs, test_output


def _wait_for_rank0(rank, world):
    """Ranks > 0 are done after the score all_gather; rank 0 still refits and tests.  Wait on the rendezvous store (a
    host-side key, no collective: nothing for a watchdog to time out) so the process group is torn down together."""
    import torch.distributed as dist
    try:
        from torch.distributed.distributed_c10d import _get_default_store
        store = _get_default_store()
        if rank == 0:
            store.set("slnlp/cli/done", "1")
        else:
            store.wait(["slnlp/cli/done"], datetime.timedelta(hours=48))
    except Exception:
        dist.barrier()


def main(argv=None):
    ap = argparse.ArgumentParser(description="SL Transformer (MI355X path)")
    ap.add_argument("--config", "-c", help="YAML file (the reference's config/config-*.yaml work unchanged)")
    for k, t in SCALAR_ARGS.items():
        ap.add_argument(f"--{k}", type=t, default=None)
    for k in DICT_ARGS:
        ap.add_argument(f"--{k}", type=json.loads, default=None, help="JSON object merged over the file's value")
    ap.add_argument("--fits_per_gpu", type=int, default=None, help="concurrent fits per GPU (not in the reference)")
    ns = vars(ap.parse_args(argv))
    path = ns.pop("config")
    args = load_config(path, {k: v for k, v in ns.items() if v is not None})
    args["workdir"] = format_dir(args.get("workdir"), **{k: v for k, v in args.items() if k != "workdir"})
    run(args)


if __name__ == "__main__":
    main()
