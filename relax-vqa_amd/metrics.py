"""Scoring a quality head: SRCC, KRCC, PLCC, RMSE on the GPU (csrc/metrics.hip) and the repeated hold-out protocol.

Follows the reference's src/model_regression.py:
  compute_correlation_metrics (:149-161), fit_logistic_regression (:143-147)   correlation_metrics: one pair pass for the two rank
                                    correlations, one persistent Levenberg-Marquardt launch for the 4-parameter logistic fit
  main()'s body for one split (:572-613)                                       evaluate_head
  main()'s repeat loop, nan_to_num, medians, median model (:548-697)           holdout_protocol
  split_train_test.process_other's train_test_split of the unique ids          holdout_split
  the greyscale rows dropped before any of it (split_train_test.py:15-21,49-50, :114-117,144;
  fine_tune.py:72-75,94; recover_median_train_test.py:23-27,50)                 drop_rows, holdout_protocol(drop_indices=...)

Out of scope, as before: plots, .mat / log writing, and the per-dataset file handling of split_train_test other than the greyscale
drop (the reports themselves are read and written by data_processing.check_greyscale).
The pure host rules (split, seeds, median model, summary) have no GPU in them and are tested on the CPU.
"""
import ctypes as C
import math

import numpy as np
import torch

MIN_N, MAX_N = 2, 131072
OUT_COUNT, KENDALL_COUNT = 17, 8
METRICS = ("SRCC", "KRCC", "PLCC", "RMSE")


# ---- pure host rules ------------------------------------------------------------------------------------------------------
def repeat_seed(i):
    """random_state of the i-th repeat (1-based): ceil(8.8 i) (model_regression.py:555)."""
    return math.ceil(8.8 * i)


def holdout_split(n, test_size=0.2, random_state=0):
    """(train_idx, test_idx) of sklearn.model_selection.train_test_split(np.arange(n), test_size=test_size,
    random_state=random_state): n_test = ceil(test_size n); the test set is the head of RandomState(seed).permutation(n),
    the train set the n - n_test indices behind it."""
    n = int(n)
    n_test = int(math.ceil(test_size * n))
    n_train = n - n_test
    if n_test < 1 or n_train < 1:
        raise ValueError(f"holdout_split: n = {n} with test_size = {test_size} leaves an empty side")
    perm = np.random.RandomState(random_state).permutation(n)
    return perm[n_test:n_test + n_train], perm[:n_test]


def group_split(groups, test_size=0.2, random_state=0):
    """Row indices (train_rows, test_rows, test_ids) when whole groups are held out: the unique ids in order of first
    appearance (pandas' unique(), as the reference's `vid` column gives them) are split by holdout_split, and a row goes
    where its id went - no id on both sides."""
    groups = np.asarray(groups)
    _, first, inverse = np.unique(groups, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")          # sorted-unique position -> appearance order
    rank = np.empty_like(order)
    rank[order] = np.arange(order.size)
    ids = groups[np.sort(first)]
    row_gid = rank[inverse.reshape(-1)]
    train_g, test_g = holdout_split(ids.size, test_size, random_state)
    is_test = np.zeros(ids.size, dtype=bool)
    is_test[test_g] = True
    return np.flatnonzero(~is_test[row_gid]), np.flatnonzero(is_test[row_gid]), ids[test_g]


def drop_rows(indices, features, mos, groups=None):
    """The reference's greyscale drop: `df.drop(index=indices).reset_index(drop=True)` on the metadata rows (mos, groups) and
    `np.delete(features, indices, axis=0)` on the feature matrix, as one rule -> (features, mos, groups) without those rows, order
    kept.  A row listed twice is dropped once (both of the reference's calls do that).  An index outside 0..n-1 raises IndexError
    naming it: df.drop raises for a label that is not there, and np.delete for an index past the end; a negative index, which
    np.delete alone would count from the end, is refused with them.  Device tensors stay on their device (index_select with the
    kept rows; no host round trip); arrays stay arrays."""
    n = int(features.shape[0])
    for name, v in (("mos", mos), ("groups", groups)):
        if v is not None and int(np.prod(tuple(v.shape))) != n:
            raise ValueError(f"drop_rows: {int(np.prod(tuple(v.shape)))} {name} values against {n} feature rows")
    idx = np.unique(np.asarray(list(indices) if not isinstance(indices, np.ndarray) else indices, dtype=np.int64).reshape(-1))
    bad = idx[(idx < 0) | (idx >= n)]
    if bad.size:
        raise IndexError(f"drop_rows: index {int(bad[0])} outside 0..{n - 1}")
    keep = np.ones(n, dtype=bool)
    keep[idx] = False
    rows = np.flatnonzero(keep)

    def take(v):
        if v is None:
            return None
        if isinstance(v, torch.Tensor):
            return v.reshape(n, *v.shape[1:]).index_select(0, torch.as_tensor(rows, dtype=torch.int64, device=v.device))
        return np.asarray(v).reshape(n, *np.asarray(v).shape[1:])[rows]
    return take(features), take(mos), take(groups)


def median_model_index(values):
    """(median, index) as main() picks the median model (:661-683): the FIRST repeat whose selection metric equals
    np.median of the nan_to_num'ed list; index None when no entry equals it (an even count between two values)."""
    values = np.nan_to_num(np.asarray(values, dtype=np.float64))
    median = float(np.median(values))
    hits = np.where(values == median)[0]
    return median, (int(hits[0]) if hits.size else None)


def summarise(per_repeat):
    """{'SRCC': [...], ...} -> ({name: nan_to_num'ed float64 array}, {name: (median, std)}) (:636-655)."""
    arrays = {k: np.nan_to_num(np.asarray(v, dtype=np.float64)) for k, v in per_repeat.items()}
    return arrays, {k: (float(np.median(a)), float(np.std(a))) for k, a in arrays.items()}


# ---- the device calls -----------------------------------------------------------------------------------------------------
def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _vec(engine, v, name):
    """Anything torch.as_tensor takes -> contiguous fp64 [n] on the engine's device (float64 input keeps every bit)."""
    if not isinstance(v, torch.Tensor):
        v = torch.as_tensor(np.asarray(v))
    v = v.detach().reshape(-1).to(engine.device, torch.float64).contiguous()
    if not MIN_N <= v.numel() <= MAX_N:
        raise ValueError(f"metrics: {name} has {v.numel()} elements, outside [{MIN_N}, {MAX_N}]")
    return v


def _pair(engine, a, b):
    a, b = _vec(engine, a, "y_true"), _vec(engine, b, "y_pred")
    if a.numel() != b.numel():
        raise ValueError(f"metrics: {a.numel()} targets against {b.numel()} predictions")
    return a, b


def kendall(engine, x, y):
    """The pair pass alone (relax_metrics_kendall): {'krcc', 'srcc', 'S', 'n1', 'n2', 'n0', 'nonfinite'}.  krcc is the very
    expression head_train.kendall_tau_b evaluates, from integer counts: the two agree bit for bit."""
    x, y = _pair(engine, x, y)
    out = np.empty(KENDALL_COUNT, dtype=np.float64)
    engine._check(engine.lib.relax_metrics_kendall(engine.h, _ptr(x), _ptr(y), int(x.numel()), C.c_void_p(out.ctypes.data), _stream()),
                  "relax_metrics_kendall")
    return {"krcc": float(out[0]), "srcc": float(out[1]), "S": int(out[2]), "n1": int(out[3]), "n2": int(out[4]), "n0": int(out[5]),
            "nonfinite": int(out[6])}


def pair_counts(engine, x, y):
    """The per-element counters of the pair pass as a host int32 [5, n] array: below / equal in x, below / equal in y, and
    the row sums of sign(dx) sign(dy) (relax_metrics_pair_counts; a test and inspection path)."""
    x, y = _pair(engine, x, y)
    counts = torch.empty((5, x.numel()), dtype=torch.int32, device=engine.device)
    engine._check(engine.lib.relax_metrics_pair_counts(engine.h, _ptr(x), _ptr(y), int(x.numel()), _ptr(counts), _stream()),
                  "relax_metrics_pair_counts")
    return counts.cpu().numpy()


def _unpack(out, fitted):
    res = {"plcc": float(out[0]), "rmse": float(out[1]), "srcc": float(out[2]), "krcc": float(out[3]), "popt": out[4:8].copy(),
           "beta": out[13:17].copy(), "converged": bool(out[9] == 1.0), "iterations": int(out[8]), "cost0": float(out[10]),
           "cost": float(out[11]), "nonfinite": int(out[12])}
    if fitted is not None:
        res["y_pred_logistic"] = fitted
    return res


def correlation_metrics(engine, y_true, y_pred, return_fitted=False):
    """compute_correlation_metrics on the device: {'plcc', 'rmse', 'srcc', 'krcc', 'popt', 'beta' (= p0), 'converged',
    'iterations', 'cost0', 'cost', 'nonfinite'} (+ 'y_pred_logistic', a device fp64 [n] tensor, with return_fitted).
    Any non-finite input gives nan metrics and its count in 'nonfinite'; it does not raise."""
    y_true, y_pred = _pair(engine, y_true, y_pred)
    n = int(y_true.numel())
    fitted = torch.empty((n,), dtype=torch.float64, device=engine.device) if return_fitted else None
    out = np.empty(OUT_COUNT, dtype=np.float64)
    rc = engine.lib.relax_metrics_correlation(engine.h, _ptr(y_true), _ptr(y_pred), n, C.c_void_p(out.ctypes.data), _ptr(fitted), _stream())
    engine._check(rc, "relax_metrics_correlation")
    return _unpack(out, fitted)


def correlation_metrics_async(engine, y_true, y_pred, out=None, fitted=None):
    """The same call with its 17 results left in a device fp64 tensor: enqueues only (tools/metrics_bench.py times it with
    device events).  y_true / y_pred must already be device fp64 vectors."""
    n = int(y_true.numel())
    out = torch.empty((OUT_COUNT,), dtype=torch.float64, device=engine.device) if out is None else out
    rc = engine.lib.relax_metrics_correlation(engine.h, _ptr(y_true), _ptr(y_pred), n, _ptr(out), _ptr(fitted), _stream())
    engine._check(rc, "relax_metrics_correlation")
    return out


def kendall_async(engine, x, y, out=None):
    out = torch.empty((KENDALL_COUNT,), dtype=torch.float64, device=engine.device) if out is None else out
    engine._check(engine.lib.relax_metrics_kendall(engine.h, _ptr(x), _ptr(y), int(x.numel()), _ptr(out), _stream()), "relax_metrics_kendall")
    return out


def device_logistic_rmse(engine, y_true, y_pred):
    """head_train.logistic_rmse without scipy: the RMSE after the device fit."""
    return correlation_metrics(engine, y_true, y_pred)["rmse"]


# ---- one split, and the protocol --------------------------------------------------------------------------------------------
def _rows(features, rows, device):
    if isinstance(features, torch.Tensor):
        return features.index_select(0, torch.as_tensor(rows, dtype=torch.int64, device=features.device))
    return np.asarray(features)[rows]


def _named(m):
    return {"SRCC": m["srcc"], "KRCC": m["krcc"], "PLCC": m["plcc"], "RMSE": m["rmse"]}


def evaluate_head(engine, features_train, mos_train, features_test, mos_test, config=None):
    """main()'s body for one split (model_regression.py:572-613): fit_head on the train set, the kept model's scores on the
    train and the test set, the four metrics of each on the device.

    The reference's quirk, kept by default: load_and_preprocess_data (:287-288) preprocesses the test matrix with an imputer
    and a MinMaxScaler fitted ON THE TEST MATRIX ITSELF, not with the train set's.  config['test_scaler'] = 'train' selects
    the conventional behaviour (the train set's scaler on both).  Both sets are scored by the inference head (load_mlp_head +
    mlp_head, BatchNorm folded), so the engine's loaded head is the fitted one (with the test-side scaler) afterwards.
    `config` goes to fit_head as it is: head_train.SIMPLE_DEFAULTS (or any config with batchnorm=False / validation='holdout') runs
    model_regression_simple.py's protocol - the plain state dict is loaded unfolded and scored the same way.

    Returns {'train': metrics, 'test': metrics, 'y_train_pred', 'y_test_pred' (host float64), 'y_train_pred_logistic',
    'y_test_pred_logistic' (host float64), 'state_dict', 'scaler', 'test_scaler', 'history'}."""
    cfg = dict(config or {})
    test_scaler_mode = cfg.pop("test_scaler", "own")
    if test_scaler_mode not in ("own", "train"):
        raise ValueError(f"evaluate_head: test_scaler {test_scaler_mode!r} (own | train)")
    ftr = torch.as_tensor(features_train).to(engine.device, torch.float32).contiguous()
    fte = torch.as_tensor(features_test).to(engine.device, torch.float32).contiguous()
    mos_train = np.asarray(mos_train.detach().cpu() if isinstance(mos_train, torch.Tensor) else mos_train, dtype=np.float64).reshape(-1)
    mos_test = np.asarray(mos_test.detach().cpu() if isinstance(mos_test, torch.Tensor) else mos_test, dtype=np.float64).reshape(-1)
    state_dict, scaler, history = engine.fit_head(ftr, mos_train, cfg)
    engine.load_mlp_head(state_dict, scaler["scale"], scaler["min"], scaler["imputer_statistics"])
    y_train_pred = engine.mlp_head(ftr).to(torch.float64)
    test_scaler = engine.fit_scaler(fte) if test_scaler_mode == "own" else scaler
    engine.load_mlp_head(state_dict, test_scaler["scale"], test_scaler["min"], test_scaler["imputer_statistics"])
    y_test_pred = engine.mlp_head(fte).to(torch.float64)
    m_train = correlation_metrics(engine, mos_train, y_train_pred, return_fitted=True)
    m_test = correlation_metrics(engine, mos_test, y_test_pred, return_fitted=True)
    return {"train": m_train, "test": m_test, "y_train_pred": y_train_pred.cpu().numpy(), "y_test_pred": y_test_pred.cpu().numpy(),
            "y_train_pred_logistic": m_train.pop("y_pred_logistic").cpu().numpy(),
            "y_test_pred_logistic": m_test.pop("y_pred_logistic").cpu().numpy(), "mos_train": mos_train, "mos_test": mos_test,
            "state_dict": state_dict, "scaler": scaler, "test_scaler": test_scaler, "history": history}


def holdout_protocol(engine, features, mos, config=None, n_repeats=21, test_size=0.2, groups=None, drop_indices=None):
    """main()'s repeated 80/20 hold-out (model_regression.py:548-697).  Repeat i = 1..n_repeats splits the unique ids of
    `groups` (default: one per row) with random_state = ceil(8.8 i) as train_test_split does, runs evaluate_head, and after
    nan_to_num takes the median and the standard deviation of each metric over the repeats.  The median model is the first
    repeat whose test-set selection metric (RMSE under select_criteria 'byrmse', KRCC otherwise) equals the median.
    drop_indices: rows dropped first by drop_rows - the Index column of a greyscale report (check_greyscale.greyscale_indices), as
    the reference's scripts drop them before they split; every row number in the result then counts in the shortened set.

    Returns a dict keyed like the reference's .mat: 'SRCC_train' ... 'RMSE_test' (float64 [n_repeats]), 'Median_KRCC' or
    'Median_RMSE', 'Test_Videos_list', 'Test_videos_Median_model'; plus 'summary' {key: (median, std)}, 'median_index',
    'median_state_dict', 'median_scaler', 'median_test_scaler', 'median_predictions' {'MOS', 'y_test_pred',
    'y_test_pred_logistic'} (the reference's score table), and 'repeats', the evaluate_head result of every repeat without its
    training history."""
    if drop_indices is not None:
        if not isinstance(features, torch.Tensor):
            features = np.asarray(features)
        features, mos, groups = drop_rows(drop_indices, features, mos if isinstance(mos, torch.Tensor) else np.asarray(mos).reshape(-1),
                                          None if groups is None else np.asarray(groups).reshape(-1))
    mos = np.asarray(mos.detach().cpu() if isinstance(mos, torch.Tensor) else mos, dtype=np.float64).reshape(-1)
    n = mos.size
    if not isinstance(features, torch.Tensor):
        features = np.asarray(features)
    if features.shape[0] != n:
        raise ValueError(f"holdout_protocol: {features.shape[0]} feature rows against {n} scores")
    groups = np.arange(n) if groups is None else np.asarray(groups).reshape(-1)
    if groups.size != n:
        raise ValueError(f"holdout_protocol: {groups.size} group ids against {n} rows")
    criterion = "RMSE" if (config or {}).get("select_criteria") == "byrmse" else "KRCC"
    per = {f"{m}_{side}": [] for side in ("train", "test") for m in METRICS}
    repeats, test_ids = [], []
    for i in range(1, int(n_repeats) + 1):
        train_rows, test_rows, ids = group_split(groups, test_size, repeat_seed(i))
        res = evaluate_head(engine, _rows(features, train_rows, engine.device), mos[train_rows],
                            _rows(features, test_rows, engine.device), mos[test_rows], config)
        for side in ("train", "test"):
            for name, value in _named(res[side]).items():
                per[f"{name}_{side}"].append(value)
        res.pop("history")
        res["train_rows"], res["test_rows"] = train_rows, test_rows
        repeats.append(res)
        test_ids.append(ids)
    arrays, summary = summarise(per)
    median, index = median_model_index(arrays[f"{criterion}_test"])
    hits = np.where(arrays[f"{criterion}_test"] == median)[0]
    out = dict(arrays)
    out.update({f"Median_{criterion}": median, "median_index": index, "summary": summary, "Test_Videos_list": test_ids,
                "Test_videos_Median_model": [test_ids[k] for k in hits] if hits.size > 1 else (test_ids[hits[0]] if hits.size else []),
                "repeats": repeats, "median_state_dict": None, "median_scaler": None, "median_test_scaler": None,
                "median_predictions": None})
    if index is not None:
        r = repeats[index]
        out.update(median_state_dict=r["state_dict"], median_scaler=r["scaler"], median_test_scaler=r["test_scaler"],
                   median_predictions={"MOS": r["mos_test"], "y_test_pred": r["y_test_pred"],
                                       "y_test_pred_logistic": r["y_test_pred_logistic"]})
    return out
