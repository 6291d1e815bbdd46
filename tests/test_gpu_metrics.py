"""-m gpu: the correlation metrics on the device (csrc/metrics.hip through the C-ABI and RelaxEngine) and the hold-out protocol.

Yardsticks and gates.
  Integer counters (S, n1, n2, per-element below / equal / row sums): a numpy count, exactly.
  krcc: head_train.kendall_tau_b, bit for bit (the same expression from the same integers).  srcc: scipy.stats.spearmanr within
  1e-12 absolute; krcc against scipy.stats.kendalltau within 1e-12 (scipy divides by the two square roots separately).
  Device fit against the host build of the same core (tests/metrics_driver.py): popt within 1e-9 relative per parameter on the
  well-conditioned set - the same operations in another summation order (a tree of 1024 lanes against one thread) move the 15
  sums by a few ulp, and the parameters follow with the condition number of the 4x4 system; 1e-9 leaves some six decades over
  fp64 rounding and stays three below what the optimiser's own tolerance (1.49e-8 on the cost) resolves.  The largest value
  seen goes to the file RELAX_METRICS_PARITY_OUT names (profiles/metrics_parity.json).
  Device fit against scipy.optimize.curve_fit: the gates of tests/test_metrics_cpu.py (rmse 1e-6 relative, plcc 1e-6 absolute
  on the well-conditioned set; on the ill-conditioned set only finiteness, cost <= cost0 and a truthful `converged`).
"""
import ctypes as C
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

import gpu_common
import metrics_cases as MC
import metrics_driver as D
from relax_vqa_amd import head_train, metrics

pytestmark = pytest.mark.gpu
SEEN = {"popt_rel": 0.0, "popt_rel_case": None, "rmse_rel_vs_scipy": 0.0, "plcc_abs_vs_scipy": 0.0, "rmse_rel_vs_host": 0.0}


@pytest.fixture(scope="module", autouse=True)
def _record_parity():
    yield
    out = os.environ.get("RELAX_METRICS_PARITY_OUT")
    if out:
        with open(out, "w") as f:
            json.dump({"what": "device fit (csrc/metrics.hip) against the host build of csrc/metrics_core.h and against "
                               "scipy.optimize.curve_fit, largest value over the 120 well-conditioned cases of tests/metrics_cases.py",
                       "gates": {"popt_rel": 1e-9, "rmse_rel_vs_scipy": 1e-6, "plcc_abs_vs_scipy": 1e-6}, "seen": SEEN}, f, indent=1,
                      sort_keys=True)


def _bits(v):
    return np.float64(v).tobytes()


def _numpy_counts(x, y, chunk=512):
    """The five per-element counters by direct comparison, a block of rows at a time."""
    n = x.size
    out = np.zeros((5, n), dtype=np.int64)
    for a in range(0, n, chunk):
        sx = np.sign(x[a:a + chunk, None] - x[None, :])
        sy = np.sign(y[a:a + chunk, None] - y[None, :])
        out[0, a:a + chunk], out[1, a:a + chunk] = (sx > 0).sum(1), (sx == 0).sum(1)
        out[2, a:a + chunk], out[3, a:a + chunk] = (sy > 0).sum(1), (sy == 0).sum(1)
        out[4, a:a + chunk] = (sx * sy).sum(1)
    return out


# ---- 7. integer counters ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["no_ties", "heavy_ties"])
@pytest.mark.parametrize("n", [2, 96, 1200, 7400])
def test_integer_counters_and_rank_correlations(n, kind):
    stats = pytest.importorskip("scipy.stats")
    eng = gpu_common.engine()
    x, y = MC.rank_case(n, kind)
    want = _numpy_counts(x, y)
    got = metrics.pair_counts(eng, x, y)
    assert np.array_equal(got.astype(np.int64), want)
    k = eng.kendall(x, y)
    n0 = n * (n - 1) // 2
    assert k["S"] == int(want[4].sum()) // 2 and k["n0"] == n0 and k["nonfinite"] == 0
    assert k["n1"] == int((want[1] - 1).sum()) // 2 and k["n2"] == int((want[3] - 1).sum()) // 2
    host = head_train.kendall_tau_b(x, y)
    assert _bits(k["krcc"]) == _bits(host), (k["krcc"], host)
    tau, rho = stats.kendalltau(x, y)[0], stats.spearmanr(x, y)[0]
    for name, a, b in (("krcc", k["krcc"], tau), ("srcc", k["srcc"], rho)):
        assert math.isnan(a) == math.isnan(b), (name, a, b)
        if not math.isnan(b):
            print(f"n {n} {kind} {name}: device {a!r} scipy {b!r} diff {abs(a - b):.2e}")
            assert abs(a - b) <= 1e-12, (name, a, b)
    core = D.host_metrics(x, y, fit=False)
    assert _bits(core["krcc"]) == _bits(k["krcc"]) and _bits(core["srcc"]) == _bits(k["srcc"])


def test_rank_correlations_at_28000_against_scipy():
    stats = pytest.importorskip("scipy.stats")
    eng = gpu_common.engine()
    rng = np.random.RandomState(28000)
    x = np.round(rng.standard_normal(28000), 3)          # a few thousand ties
    y = 0.7 * x + 0.7 * rng.standard_normal(28000)
    k = eng.kendall(x, y)
    tau, rho = stats.kendalltau(x, y)[0], stats.spearmanr(x, y)[0]
    print(f"n 28000: krcc {k['krcc']!r} scipy {tau!r}; srcc {k['srcc']!r} scipy {rho!r}; n1 {k['n1']}")
    assert abs(k["krcc"] - tau) <= 1e-12 and abs(k["srcc"] - rho) <= 1e-12
    assert k["n1"] > 0 and k["n2"] == 0 and k["n0"] == 28000 * 27999 // 2


def test_constant_and_monotone_vectors():
    eng = gpu_common.engine()
    for n in (2, 3, 240):
        x, y = MC.rank_case(n, "constant")
        k = eng.kendall(x, y)
        assert math.isnan(k["krcc"]) and math.isnan(k["srcc"]) and k["n2"] == k["n0"]
        x, y = MC.rank_case(n, "monotone")
        k = eng.kendall(x, y)
        assert k["krcc"] == 1.0 and k["srcc"] == 1.0
        x, y = MC.rank_case(n, "anti_monotone")
        k = eng.kendall(x, y)
        assert k["krcc"] == -1.0 and k["srcc"] == -1.0


def test_non_finite_input_and_size_limits():
    eng = gpu_common.engine()
    r = eng.correlation_metrics([1.0, float("nan"), 3.0, 4.0, float("inf")], [1.0, 2.0, float("-inf"), 4.0, 5.0], return_fitted=True)
    assert r["nonfinite"] == 3 and not r["converged"] and r["iterations"] == 0
    for key in ("plcc", "rmse", "srcc", "krcc"):
        assert math.isnan(r[key]), key
    assert np.isnan(r["popt"]).all() and torch.isnan(r["y_pred_logistic"]).all()
    assert eng.kendall([1.0, float("nan")], [1.0, 2.0])["nonfinite"] == 1
    v = torch.zeros(4, dtype=torch.float64, device=eng.device)
    out = np.zeros(17)
    for n in (1, 0, -5, metrics.MAX_N + 1):   # refused before anything is read: the invalid-argument status
        rc = eng.lib.relax_metrics_correlation(eng.h, C.c_void_p(v.data_ptr()), C.c_void_p(v.data_ptr()), n, C.c_void_p(out.ctypes.data),
                                               None, None)
        assert rc == -1, (n, rc)
        rc = eng.lib.relax_metrics_kendall(eng.h, C.c_void_p(v.data_ptr()), C.c_void_p(v.data_ptr()), n, C.c_void_p(out.ctypes.data), None)
        assert rc == -1, (n, rc)
    with pytest.raises(ValueError):
        eng.correlation_metrics([1.0], [2.0])


# ---- 8. the device fit -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("args", [c[1] for c in MC.well_conditioned()], ids=[c[0] for c in MC.well_conditioned()])
def test_device_fit_well_conditioned(args):
    pytest.importorskip("scipy.optimize")
    eng = gpu_common.engine()
    y_true, y_pred = MC.fit_case(*args)
    dev = eng.correlation_metrics(y_true, y_pred, return_fitted=True)
    host = D.host_metrics(y_true, y_pred, ranks=False)
    _, rmse, plcc = MC.scipy_fit(y_true, y_pred)
    rel = float(np.max(np.abs(dev["popt"] - host["popt"]) / np.abs(host["popt"])))
    rmse_rel, plcc_abs = abs(dev["rmse"] - rmse) / rmse, abs(dev["plcc"] - plcc)
    print(f"device fit {args}: popt rel vs host core {rel:.2e}; rmse rel vs scipy {rmse_rel:.2e}; plcc abs vs scipy {plcc_abs:.2e}; "
          f"iterations {dev['iterations']} (host {host['iterations']})")
    if rel > SEEN["popt_rel"]:
        SEEN["popt_rel"], SEEN["popt_rel_case"] = rel, list(map(str, args))
    SEEN["rmse_rel_vs_scipy"] = max(SEEN["rmse_rel_vs_scipy"], rmse_rel)
    SEEN["plcc_abs_vs_scipy"] = max(SEEN["plcc_abs_vs_scipy"], plcc_abs)
    SEEN["rmse_rel_vs_host"] = max(SEEN["rmse_rel_vs_host"], abs(dev["rmse"] - host["rmse"]) / host["rmse"])
    assert dev["converged"] and dev["nonfinite"] == 0 and dev["cost"] <= dev["cost0"]
    assert rel <= 1e-9, rel
    assert rmse_rel <= 1e-6 and plcc_abs <= 1e-6, (rmse_rel, plcc_abs)
    assert np.array_equal(dev["beta"][[0, 1, 3]], [y_true.max(), y_true.min(), 0.5]) and abs(dev["beta"][2] - y_pred.mean()) <= 1e-12 * abs(y_pred.mean())
    fitted = dev["y_pred_logistic"].cpu().numpy()
    assert np.allclose(fitted, MC.logistic(y_pred, *dev["popt"]), rtol=1e-12, atol=0)
    assert abs(dev["rmse"] - math.sqrt(np.mean((y_true - fitted) ** 2))) <= 1e-12 * dev["rmse"]


@pytest.mark.parametrize("args", [c[1] for c in MC.ill_conditioned()], ids=[c[0] for c in MC.ill_conditioned()])
def test_device_fit_ill_conditioned(args):
    pytest.importorskip("scipy.optimize")
    eng = gpu_common.engine()
    y_true, y_pred = MC.fit_case(*args)
    dev = eng.correlation_metrics(y_true, y_pred, return_fitted=True)
    _, rmse, _ = MC.scipy_fit(y_true, y_pred)
    print(f"ill-conditioned {args}: device rmse {dev['rmse']:.12g} scipy {rmse:.12g} converged {dev['converged']} iterations {dev['iterations']}")
    for key in ("plcc", "rmse", "srcc", "krcc", "cost0", "cost"):
        assert math.isfinite(dev[key]), key
    assert np.isfinite(dev["popt"]).all() and torch.isfinite(dev["y_pred_logistic"]).all()
    assert dev["cost"] <= dev["cost0"] and 0 <= dev["iterations"] <= 400
    if dev["converged"]:
        assert MC.stopping_rule_holds(y_true, y_pred, dev["popt"], 10.0)
    else:
        assert not MC.stopping_rule_holds(y_true, y_pred, dev["popt"], 0.1)


# ---- 9. reproducibility -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [96, 7000, 28000])
def test_two_calls_are_bit_identical(n):
    eng = gpu_common.engine()
    y_true, y_pred = MC.fit_case(n, "mos5", 0.3, True, 11)
    yt = torch.as_tensor(y_true).to(eng.device)
    yp = torch.as_tensor(y_pred).to(eng.device)
    runs = []
    for _ in range(2):
        fitted = torch.empty(n, dtype=torch.float64, device=eng.device)
        out = metrics.correlation_metrics_async(eng, yt, yp, fitted=fitted)   # `out` in device memory: the enqueue-only form
        runs.append((out.cpu().numpy().tobytes(), fitted.cpu().numpy().tobytes()))
    assert runs[0] == runs[1]
    host_form = eng.correlation_metrics(yt, yp)                              # `out` in host memory: the same numbers
    dev_form = np.frombuffer(runs[0][0], dtype=np.float64)
    assert _bits(host_form["rmse"]) == _bits(dev_form[1]) and _bits(host_form["krcc"]) == _bits(dev_form[3])
    assert host_form["popt"].tobytes() == dev_form[4:8].tobytes()


# ---- 10. / 11. fit_head ----------------------------------------------------------------------------------------------------------------
def _small_set(seed=0, n=240, F=200):
    rng = np.random.RandomState(seed)
    x = rng.uniform(0, 10, size=(n, F)).astype(np.float32)
    mos = (3 + np.sin(x[:, 0] * 0.5) + 0.1 * x[:, 1] - 0.02 * x[:, 2] ** 2 + 0.05 * rng.standard_normal(n)).astype(np.float32)
    return x, mos


SMALL_CFG = dict(n_splits=3, epochs=12, hidden_features=128, batch_size=64, seed=3)


def test_fit_head_selection_is_unchanged(monkeypatch):
    eng = gpu_common.engine()
    x, mos = _small_set()
    seen = []
    real = head_train._evaluate_set

    def recording(tr, xp, y, rows, which, cfg):
        loss, pred = real(tr, xp, y, rows, which, cfg)
        seen.append((np.asarray(rows).copy(), pred.copy()))
        return loss, pred
    monkeypatch.setattr(head_train, "_evaluate_set", recording)
    _, _, hist = eng.fit_head(torch.as_tensor(x).to(eng.device), mos, dict(SMALL_CFG, select_criteria="bykrcc"))
    y64 = mos.astype(np.float64)
    host = [head_train.kendall_tau_b(y64[rows], pred) for rows, pred in seen]
    flat = [m for fold in hist["metric"] for m in fold]
    assert len(flat) == len(host) and len(flat) >= 3 * 9
    assert [_bits(a) for a in flat] == [_bits(b) for b in host]
    best, best_metric, k = None, float("-inf"), 0   # the selection rule on the host numbers: the first strictly larger one wins
    for fold, fold_metrics in enumerate(hist["metric"]):
        for epoch in range(len(fold_metrics)):
            if host[k] > best_metric:
                best_metric, best = host[k], (fold, epoch, host[k])
            k += 1
    assert hist["best"] == best


def test_byrmse_runs_without_scipy(monkeypatch):
    eng = gpu_common.engine()
    x, mos = _small_set(1)
    for name in [m for m in sys.modules if m == "scipy" or m.startswith("scipy.")]:
        monkeypatch.delitem(sys.modules, name)
    monkeypatch.setitem(sys.modules, "scipy", None)
    monkeypatch.setitem(sys.modules, "scipy.optimize", None)
    with pytest.raises(ImportError):
        import scipy.optimize  # noqa: F401
    for cfg in (dict(logistic_fit="device"), dict()):   # asked for, and taken because curve_fit cannot be imported
        _, _, hist = eng.fit_head(torch.as_tensor(x).to(eng.device), mos, dict(SMALL_CFG, epochs=6, select_criteria="byrmse", **cfg))
        flat = [m for fold in hist["metric"] for m in fold]
        assert len(flat) >= 3 * 4 and all(math.isfinite(m) and m > 0 for m in flat)
        assert hist["best"][2] == min(flat)


def test_byrmse_device_fit_tracks_scipy():
    pytest.importorskip("scipy.optimize")
    eng = gpu_common.engine()
    x, mos = _small_set(2)
    feats = torch.as_tensor(x).to(eng.device)
    cfg = dict(SMALL_CFG, epochs=6, select_criteria="byrmse")
    _, _, h_dev = eng.fit_head(feats, mos, dict(cfg, logistic_fit="device"))
    _, _, h_host = eng.fit_head(feats, mos, cfg)
    for a, b in zip([m for f in h_dev["metric"] for m in f], [m for f in h_host["metric"] for m in f]):
        print(f"byrmse per-epoch metric: device {a!r} scipy {b!r}")
    assert len(h_dev["metric"]) == len(h_host["metric"]) == 3


# ---- 12. the protocol --------------------------------------------------------------------------------------------------------------------
def test_holdout_protocol_end_to_end():
    eng = gpu_common.engine()
    x, mos32 = _small_set(4, n=240, F=512)
    mos = mos32.astype(np.float64) + 1e-9 * np.arange(240)     # float64 scores that fp32 cannot hold: they must arrive unrounded
    cfg = dict(n_splits=3, epochs=8, hidden_features=128, batch_size=64, seed=1)
    res = eng.holdout_protocol(torch.as_tensor(x).to(eng.device), mos, cfg, n_repeats=3)
    keys = {f"{m}_{side}" for m in metrics.METRICS for side in ("train", "test")} | {
        "Median_KRCC", "median_index", "summary", "Test_Videos_list", "Test_videos_Median_model", "repeats", "median_state_dict",
        "median_scaler", "median_test_scaler", "median_predictions"}
    assert keys <= set(res)
    for i, rep in enumerate(res["repeats"], start=1):
        train_rows, test_rows = metrics.holdout_split(240, 0.2, metrics.repeat_seed(i))
        assert np.array_equal(rep["train_rows"], np.sort(train_rows)) and np.array_equal(rep["test_rows"], np.sort(test_rows))
        assert rep["mos_test"].dtype == np.float64 and np.array_equal(rep["mos_test"], mos[rep["test_rows"]])
        assert len(rep["y_test_pred"]) == 48 and len(rep["y_train_pred"]) == 192
        for side in ("train", "test"):
            again = eng.correlation_metrics(rep[f"mos_{side}"], rep[f"y_{side}_pred"], return_fitted=True)
            for name, key in (("SRCC", "srcc"), ("KRCC", "krcc"), ("PLCC", "plcc"), ("RMSE", "rmse")):
                assert _bits(again[key]) == _bits(rep[side][key])
                assert _bits(np.nan_to_num(again[key])) == _bits(res[f"{name}_{side}"][i - 1])
            assert np.array_equal(again["y_pred_logistic"].cpu().numpy(), rep[f"y_{side}_pred_logistic"])
        print(f"repeat {i}: train {metrics._named(rep['train'])} test {metrics._named(rep['test'])}")
    krcc = res["KRCC_test"]
    assert res["Median_KRCC"] == float(np.median(krcc))
    assert res["median_index"] == int(np.where(krcc == np.median(krcc))[0][0])
    chosen = res["repeats"][res["median_index"]]
    assert res["median_state_dict"] is chosen["state_dict"] and np.array_equal(res["median_predictions"]["y_test_pred"], chosen["y_test_pred"])
    assert set(res["median_predictions"]) == {"MOS", "y_test_pred", "y_test_pred_logistic"}
    for key in ("SRCC_test", "RMSE_train"):
        assert res["summary"][key] == (float(np.median(res[key])), float(np.std(res[key])))
    # the reference's quirk (the test matrix scaled by its own range) is the default; the train set's scaler is a switch
    conv = eng.evaluate_head(x[:192], mos[:192], x[192:], mos[192:], dict(cfg, test_scaler="train"))
    own = eng.evaluate_head(x[:192], mos[:192], x[192:], mos[192:], cfg)
    assert np.array_equal(conv["test_scaler"]["scale"], conv["scaler"]["scale"])
    assert np.array_equal(own["scaler"]["scale"], conv["scaler"]["scale"]) and not np.array_equal(own["test_scaler"]["scale"], own["scaler"]["scale"])
    assert np.array_equal(own["test_scaler"]["scale"], eng.fit_scaler(torch.as_tensor(x[192:]).to(eng.device))["scale"])
