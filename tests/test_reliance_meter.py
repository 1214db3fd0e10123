"""RelianceMeter (src/robustness.py) without a GPU, through update_rows only: result() against a
from-scratch fp64 analysis (np.corrcoef for Pearson's R, per-repeat accuracy via mean / std) on the
stack of tests/golden/robustness_small_t16.npz with seeded labels -- the rows and hit sums fed to the
meter are made by the numpy restatement of include/mmu.h's table (test_robustness_summary_gpu.py
summary_ref) -- batching, merge, pickle, a world-2 gloo exchange, and the new flags of
eval_mmbt_robustness.py and train.py.
"""
import argparse
import os
import pickle

import numpy as np
import pytest
import torch
import torch.distributed as dist

from test_dp_gloo import _spawn
from test_robustness_summary_gpu import COLUMNS, rows_and_hits, summary_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "robustness_small_t16.npz")
TOL = 1e-12


def golden_stack(S=24, seed=4):
    """[S, 9, 1, 101] f32: the golden file's 3 samples (n_repeats = 3) and seeded perturbations of them, so
    that the set has enough samples for a correlation; labels: the full forward's class for two samples
    in three, a seeded class for the rest"""
    g = np.random.default_rng(seed)
    d = np.load(GOLDEN)
    preds, n = d["preds"], int(d["n_repeats"])
    assert preds.shape == (3, 3 + 2 * n, 101)
    reps = [preds]
    while sum(len(r) for r in reps) < S:
        reps.append(preds + (0.3 * g.standard_normal(preds.shape)).astype(np.float32))
    z = np.concatenate(reps)[:S, :, None, :].astype(np.float32)
    y = np.where(np.arange(S) % 3 < 2, z[:, 0, 0].argmax(-1), g.integers(0, 101, S)).astype(np.int64)
    return z, y, n


def fed_meter(rows, hits, n, cuts=()):
    from src.robustness import RelianceMeter
    m = RelianceMeter(n)
    edges = [0] + list(cuts) + [len(rows)]
    for a, b in zip(edges[:-1], edges[1:]):
        m.update_rows(rows[a:b], hits[a:b].sum(0))
    return m


def per_sample_hits(ref):
    return ref["hit"].astype(np.float64)               # [S, V]; a batch's hit sums are its rows' sum


def assert_results_equal(a, b, tol=TOL):
    assert set(a) == set(b)
    for k in a:
        if isinstance(a[k], dict):
            assert_results_equal(a[k], b[k], tol)
        elif a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, k
        else:
            assert abs(a[k] - b[k]) <= tol, (k, a[k], b[k])


def test_result_against_a_from_scratch_analysis():
    z, y, n = golden_stack()
    S, V = z.shape[:2]
    ref = summary_ref(z, y, np.float64)
    rows, hits = rows_and_hits(ref)
    m = fed_meter(rows, per_sample_hits(ref), n)
    assert np.array_equal(m.hits, hits)
    res = m.result()
    assert set(res) == {"n", "acc", "corr", "js_corr"} | set(COLUMNS)

    # from scratch, on the probabilities
    zz = z[:, :, 0].astype(np.float64)
    e = np.exp(zz - zz.max(-1, keepdims=True))
    p = e / e.sum(-1, keepdims=True)
    pl = p[np.arange(S), :, y]                                           # [S, V]
    dp = pl - pl[:, :1]
    pred = zz.argmax(-1)
    acc = (pred == y[:, None]).mean(0)                                   # per variant, a fraction
    img, txt = slice(3, 3 + n), slice(3 + n, V)
    assert res["n"] == S
    assert abs(res["acc"]["full"] - acc[0]) <= TOL and abs(res["acc"]["image"] - acc[1]) <= TOL
    assert abs(res["acc"]["text"] - acc[2]) <= TOL
    for name, sl in (("image_control", img), ("text_control", txt)):
        assert abs(res["acc"][name]["mean"] - acc[sl].mean()) <= TOL
        assert abs(res["acc"][name]["std"] - acc[sl].std()) <= TOL
    for mod, v, sl in (("image", 1, img), ("text", 2, txt)):
        r = np.corrcoef(dp[:, v], dp[:, sl].mean(1))[0, 1]
        assert res["corr"][mod] is not None and abs(res["corr"][mod] - r) <= TOL, (mod, res["corr"][mod], r)
        rj = np.corrcoef(ref["js"][:, v], ref["js"][:, sl].mean(1))[0, 1]
        assert abs(res["js_corr"][mod] - rj) <= TOL
    for i, c in enumerate(COLUMNS):
        assert abs(res[c] - rows[:, i].mean()) <= TOL, c
    assert abs(res["p_full"] - pl[:, 0].mean()) <= TOL
    assert abs(res["dp_text_control"] - dp[:, txt].mean()) <= TOL
    assert abs(res["sd_image_control"] - dp[:, img].std(1).mean()) <= TOL
    ps = m.per_sample()
    assert list(ps) == list(COLUMNS) and all(ps[c].dtype == np.float64 and ps[c].shape == (S,) for c in ps)
    assert np.array_equal(ps["dp_image"], rows[:, 1])


def test_corr_is_none_for_constant_columns_and_one_sample():
    from src.robustness import RelianceMeter, pearson
    z, y, n = golden_stack()
    ref = summary_ref(z, y, np.float64)
    rows, _ = rows_and_hits(ref)
    one = fed_meter(rows[:1], per_sample_hits(ref)[:1], n).result()
    assert one["n"] == 1 and one["corr"] == {"image": None, "text": None}
    assert one["js_corr"] == {"image": None, "text": None}
    const = rows.copy()
    const[:, COLUMNS.index("dp_image")] = 0.25                           # one side constant
    const[:, COLUMNS.index("js_text_control")] = 0.0
    res = fed_meter(const, per_sample_hits(ref), n).result()
    assert res["corr"]["image"] is None and res["corr"]["text"] is not None
    assert res["js_corr"]["text"] is None and res["js_corr"]["image"] is not None
    assert pearson([1.0, 2.0, 4.0], [2.0, 4.0, 8.0]) == pytest.approx(1.0, abs=TOL)
    assert pearson([1.0, 2.0, 4.0], [-2.0, -4.0, -8.0]) == pytest.approx(-1.0, abs=TOL)   # signed
    assert pearson([0.1] * 5, [1.0, 2.0, 3.0, 4.0, 5.0]) is None
    assert pearson([3.0], [4.0]) is None and pearson([], []) is None
    empty = RelianceMeter(n).result()
    assert empty["n"] == 0 and empty["corr"] == {"image": None, "text": None}
    # what the entry point writes is strict JSON: the undefined figures are null, nothing else moves
    import json
    from src.robustness import json_safe
    assert np.isnan(empty["p_full"])
    with pytest.raises(ValueError):
        json.dumps(empty, allow_nan=False)
    safe = json.loads(json.dumps(json_safe(empty), allow_nan=False))
    assert safe["p_full"] is None and safe["js_text"] is None and safe["n"] == 0
    assert safe["acc"]["image_control"] == {"mean": 0.0, "std": 0.0}
    assert json_safe(res) == res and json_safe({"a": [1.5, float("inf"), "x"]}) == {"a": [1.5, None, "x"]}


def test_batches_merge_and_pickle():
    from src.robustness import RelianceMeter
    z, y, n = golden_stack()
    ref = summary_ref(z, y, np.float64)
    rows, _ = rows_and_hits(ref)
    ph = per_sample_hits(ref)
    whole = fed_meter(rows, ph, n).result()
    assert_results_equal(fed_meter(rows, ph, n, cuts=(5, 6)).result(), whole)        # three batches
    a, b = fed_meter(rows[:11], ph[:11], n, cuts=(4,)), fed_meter(rows[11:], ph[11:], n)
    merged = RelianceMeter(n)
    merged.merge(a.state())
    merged.merge(b.state())
    assert_results_equal(merged.result(), whole)
    assert np.array_equal(merged.per_sample()["js_text"], rows[:, COLUMNS.index("js_text")])
    st = pickle.loads(pickle.dumps(a.state()))
    assert set(st) == {"n_repeats", "rows", "hits"} and all(
        type(v) in (int, np.ndarray) for v in st.values())                            # plain numpy
    again = RelianceMeter(n)
    again.merge(st)
    assert_results_equal(again.result(), a.result(), 0.0)
    merged.merge(RelianceMeter(n).state())                                            # an empty shard
    assert_results_equal(merged.result(), whole)
    with pytest.raises(ValueError, match="n_repeats"):
        RelianceMeter(n + 1).merge(st)
    with pytest.raises(ValueError, match="stats must be"):
        RelianceMeter(n).update_rows(rows[:, :5], ph[:1].sum(0))
    with pytest.raises(ValueError, match="hits must be"):
        RelianceMeter(n).update_rows(rows, ph.sum(0)[:-1])


def _gloo_worker(rank, world, port, q):
    """each rank feeds its half of the rows, then gather_meters: both must hold the whole set's result"""
    try:
        import sys
        here = os.path.dirname(os.path.abspath(__file__))
        sys.path[:0] = [os.path.join(os.path.dirname(here), "multi-modal-uncertainty_amd"), os.path.dirname(here), here]
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        dist.init_process_group("gloo", rank=rank, world_size=world)
        from src.robustness import gather_meters
        z, y, n = golden_stack()
        ref = summary_ref(z, y, np.float64)
        rows, _ = rows_and_hits(ref)
        ph = per_sample_hits(ref)
        half = slice(0, 13) if rank == 0 else slice(13, None)
        whole = gather_meters(fed_meter(rows[half], ph[half], n))
        q.put((rank, whole.result(), whole.per_sample()["dp_image"]))
        dist.destroy_process_group()
    except Exception:  # pragma: no cover - reported to the parent
        import traceback
        q.put((rank, "ERR", traceback.format_exc()))


def test_world_2_exchange_gives_every_rank_the_whole_set():
    z, y, n = golden_stack()
    ref = summary_ref(z, y, np.float64)
    rows, _ = rows_and_hits(ref)
    whole = fed_meter(rows, per_sample_hits(ref), n).result()
    res = _spawn(_gloo_worker, 2)
    for rank, result, dp_image in res:
        assert_results_equal(result, whole)
        assert np.array_equal(dp_image, rows[:, 1])                      # merged in rank order
    assert_results_equal(res[0][1], res[1][1], 0.0)                      # and the ranks log the same values


def test_a_single_process_keeps_its_meter():
    from src.robustness import RelianceMeter, gather_meters
    m = RelianceMeter(2)
    assert gather_meters(m) is m


def test_history_columns():
    from src.robustness import REL_COLUMNS, RelianceCallback, reliance_logs
    z, y, n = golden_stack()
    ref = summary_ref(z, y, np.float64)
    rows, _ = rows_and_hits(ref)
    res = fed_meter(rows, per_sample_hits(ref), n).result()
    logs = reliance_logs(res, "val")
    assert list(logs) == ["val_rel_" + c for c in REL_COLUMNS] == [
        "val_rel_corr_image", "val_rel_corr_text", "val_rel_acc_full", "val_rel_acc_image", "val_rel_acc_text",
        "val_rel_acc_image_control", "val_rel_acc_text_control", "val_rel_js_image", "val_rel_js_text"]
    assert logs["val_rel_acc_full"] == 100.0 * res["acc"]["full"]        # percent, like the framework's acc
    assert logs["val_rel_acc_text_control"] == 100.0 * res["acc"]["text_control"]["mean"]
    assert logs["val_rel_corr_text"] == res["corr"]["text"] and logs["val_rel_js_image"] == res["js_image"]
    one = reliance_logs(fed_meter(rows[:1], per_sample_hits(ref)[:1], n).result(), "test")
    assert np.isnan(one["test_rel_corr_image"]) and all(isinstance(v, float) for v in one.values())
    # a skipped epoch: NaN in every column, nothing run
    cb = RelianceCallback(model=None, loader=None, device="cpu", n_repeats=n, every=2)
    logs = {"epoch": 1}
    cb.on_epoch_end(1, logs)
    assert list(logs) == ["epoch"] + cb.columns() and all(np.isnan(logs[c]) for c in cb.columns())
    with pytest.raises(ValueError, match="every"):
        RelianceCallback(None, None, "cpu", every=0)


# ------------------------------------------------------------------------------- flags
def test_eval_entry_point_parses_summary():
    import eval_mmbt_robustness as E
    p = argparse.ArgumentParser()
    E.get_args(p)
    base = ["--save_path", "out", "--phase", "val", "--batch_size", "2", "--checkpoint_path", "m.pt"]
    assert p.parse_args(base).summary is False
    assert p.parse_args(base + ["--summary"]).summary is True


def parse_train(argv):
    import train as T
    p = argparse.ArgumentParser()
    T.get_args(p)
    return p.parse_args(["--save_path", "out", "--framework", "mmbt", "--dataset", "food101"] + argv)


def test_train_flags_default_off_and_leave_run_meta_alone():
    import train as T
    a = parse_train([])
    assert (a.reliance_every, a.reliance_repeats, a.reliance_steps) == (0, 20, None)
    assert T.reliance_callback(a, None, None, "cpu") is None
    T.check_reliance_args(a)
    assert T.run_meta(a) == {"framework": "mmbt", "dataset": "food101", "model_type": "Vanilla", "seed": 42,
                             "batch_size": 128, "synthetic": 0, "deterministic": False}
    old = argparse.Namespace(**{k: v for k, v in vars(a).items() if not k.startswith("reliance_")})
    assert T.run_meta(old) == T.run_meta(a) and T.reliance_callback(old, None, None, "cpu") is None


def test_train_flags_on():
    import train as T
    from src.robustness import RelianceCallback
    a = parse_train(["--reliance_every", "2", "--reliance_repeats", "4", "--reliance_steps", "3", "--seed", "7"])
    assert (a.reliance_every, a.reliance_repeats, a.reliance_steps) == (2, 4, 3)
    meta = T.run_meta(a)
    assert (meta["reliance_every"], meta["reliance_repeats"], meta["reliance_steps"]) == (2, 4, 3)
    assert list(meta)[:7] == list(T.run_meta(parse_train([])))
    cb = T.reliance_callback(a, "model", "loader", "cpu")
    assert isinstance(cb, RelianceCallback)
    assert (cb.rel_model, cb.loader, cb.n_repeats, cb.every, cb.steps, cb.seed, cb.prefix) == (
        "model", "loader", 4, 2, 3, 7, "val")
    T.check_reliance_args(a)
    # in front of the history callbacks, on the device the model was moved to -- and only on a GPU
    default = ["history", "csv"]
    both = T.with_reliance(a, "model", "loader", torch.device("cuda:1"), default)
    assert len(both) == 3 and isinstance(both[0], RelianceCallback) and both[1:] == default
    assert both[0].device == torch.device("cuda:1") and default == ["history", "csv"]
    assert T.with_reliance(a, "model", "loader", torch.device("cuda:0"), [])[0].loader == "loader"   # ranks != 0
    for device in (None, torch.device("cpu")):
        with pytest.raises(SystemExit, match="--use_gpu"):
            T.with_reliance(a, "model", "loader", device, default)
    off = parse_train([])
    assert T.with_reliance(off, "model", "loader", None, default) is default
    a.framework = "flava"
    with pytest.raises(SystemExit, match="mmbt only"):
        T.check_reliance_args(a)
    with pytest.raises(SystemExit, match="mmbt only"):
        T.main(["--save_path", "out", "--framework", "flava", "--reliance_every", "1"])
