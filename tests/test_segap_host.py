"""Temporal detection mAP without a GPU: the restatement tests/segap_ref.py against the recorded results of the reference
(tests/golden/segap.npz, written by tests/golden/make_golden_segap.py), the JSON loaders, the label remap with its drop rule,
the drop-in names' signatures, and the C entry points' argument checks."""
import ctypes
import inspect
import json
import os

import numpy as np
import pytest
import torch

from otpose_amd import hip, ops, segmetrics
from tests import segap_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "segap.npz")
T_SETS = (1, 5, 10)


@pytest.fixture(scope="module")
def z():
    return dict(np.load(GOLDEN))


def e2e_preds(z):
    return {"video-id": z["e_pred_vid"].tolist(), "t-start": z["e_pred_t-start"], "t-end": z["e_pred_t-end"],
            "label": z["e_pred_label"], "score": z["e_pred_score"]}


def write_pred_json(path, preds):
    db = {}
    for v, s, e, l, p in zip(preds["video-id"], preds["t-start"], preds["t-end"], preds["label"], preds["score"]):
        db.setdefault(v, []).append({"segment": [float(s), float(e)], "label_id": int(l), "scores": float(p)})
    with open(path, "w") as f:
        json.dump({"database": db}, f)


def test_the_file_holds_the_cases_and_the_reference_wrote_it(z):
    assert str(z["yardstick"]) == "reference"
    cap = hip.CONSTANTS["OTP_SEG_AP_LDS_GT"]
    sizes = list(zip(np.diff(z["m_gt_offsets"]).tolist(), np.diff(z["m_pred_offsets"]).tolist()))
    assert sizes[:9] == [(0, 5), (1, 0), (1, 1), (2, 7), (63, 200), (64, 200), (65, 200), (cap + 1, 40), (4, 1025)]
    assert bool(z["m_nan_group"]) == (len(sizes) == 10)
    if z["m_nan_group"]:                                        # one zero-length prediction on one identical ground truth
        assert sizes[9] == (1, 1) and np.array_equal(z["m_gt_seg"][-1], z["m_pred_seg"][-1]) and z["m_gt_seg"][-1, 0] == z["m_gt_seg"][-1, 1]
    assert np.diff(z["a_class_offsets"]).tolist() == [0, 1, 255, 256, 257, 5000, 30, 20]
    assert [len(z[f"thresholds_T{T}"]) for T in T_SETS] == [1, 5, 10]
    assert os.path.getsize(GOLDEN) < 400 * 1024


@pytest.mark.parametrize("T", T_SETS)
def test_restatement_reproduces_the_recorded_match_batch(z, T):
    thr = z[f"thresholds_T{T}"]
    match = R.match_groups(z["m_pred_seg"], z["m_pred_offsets"], z["m_gt_seg"], z["m_gt_offsets"], thr)
    assert np.array_equal(match, z[f"m_match_T{T}"]) and match.dtype == np.int32
    if z["m_nan_group"]:
        assert (match[:, -1] == 0).all()                        # 0 / 0 is not < thr: a true positive, as in the reference
    # the batch as one class whose videos are the groups: the reference's AP of it
    gv = np.repeat(np.arange(len(z["m_gt_offsets"]) - 1), np.diff(z["m_gt_offsets"]))
    pv = np.repeat(np.arange(len(z["m_pred_offsets"]) - 1), np.diff(z["m_pred_offsets"]))
    ap, m2, tp, order = R.class_ap(gv, z["m_gt_seg"], pv, z["m_pred_seg"], z["m_score"], thr)
    assert ap.tobytes() == z[f"m_ap_T{T}"].tobytes()
    assert np.array_equal(m2, match[:, order]) and np.array_equal(tp, m2 >= 0)


def test_restatement_reproduces_the_recorded_ap_case(z):
    off, order = z["a_class_offsets"], z["a_order"]
    for c in range(len(off) - 1):
        rows = order[off[c]:off[c + 1]]
        ap = R.ap_from_tp(z["a_match"][:, rows] >= 0, z["a_npos"][c]) if len(rows) else np.zeros(5)
        assert ap.tobytes() == z["a_ap"][:, c].tobytes()
    assert (z["a_ap"][:, 6] == 1.0).all() and (z["a_ap"][:, 7] == 0.0).all() and (z["a_ap"][:, 0] == 0.0).all()


def test_loaders_remap_and_restatement_on_the_end_to_end_case(z, tmp_path):
    path = str(tmp_path / "gt.json")
    with open(path, "w") as f:
        f.write(str(z["e_gt_json"]))
    everything = segmetrics.load_gt_seg_from_json(path)
    gt = segmetrics.load_gt_seg_from_json(path, split="validation")
    assert list(gt) == ["video-id", "t-start", "t-end", "label"]
    assert gt["t-start"].dtype == np.float64 and gt["label"].dtype == np.int64
    assert len(set(everything["video-id"])) == 11 and len(set(gt["video-id"])) == 8     # video_08 has no annotation
    assert 0 < len(gt["label"]) < len(everything["label"])
    preds = e2e_preds(z)
    for T, key in ((5, "e_ap"), (10, "e_ap10")):
        ap, mAP, avg = R.detection_ap(gt, preds, z[f"thresholds_T{T}"])
        assert ap.tobytes() == z[key].tobytes()
        assert R.kernel_tables(gt, preds, z[f"thresholds_T{T}"])["ap"].tobytes() == z[key].tobytes()
    assert (z["e_ap"][:, 3] == 0).all() and (z["e_ap"][:, [0, 1, 2, 4, 5]] > 0).all()     # label 7 has no predictions

    pred_path = str(tmp_path / "pred.json")
    write_pred_json(pred_path, preds)
    loaded = segmetrics.load_pred_seg_from_json(pred_path)
    assert list(loaded) == ["video-id", "t-start", "t-end", "label", "score"]
    assert sorted(zip(loaded["video-id"], loaded["t-start"], loaded["t-end"], loaded["label"], loaded["score"])) == \
        sorted(zip(preds["video-id"], preds["t-start"], preds["t-end"], preds["label"], preds["score"]))

    # the constructor groups the ground truth with torch operations only: it runs wherever it is told to
    det = segmetrics.ANETdetection(path, split="validation", device="cpu")
    assert det.activity_index == {int(l): i for i, l in enumerate(z["e_labels"])}
    assert det.dataset_name == "gt" and det.ap is None and np.array_equal(det.tiou_thresholds, np.linspace(0.1, 0.5, 5))
    assert np.array_equal(det.ground_truth["label"], R.remap(gt["label"], z["e_labels"])[0])
    assert det._gt.npos.tolist() == np.bincount(det.ground_truth["label"]).tolist()
    assert det._gt.n_groups == 9 * 6 and det._gt.offsets[-1].item() == len(gt["label"])
    with pytest.raises(NotImplementedError):                    # no CPU path for the metric itself
        det.evaluate(preds, verbose=False)
    same = segmetrics.ANETdetection(None, ground_truth=gt, device="cpu")
    assert same.activity_index == det.activity_index and torch.equal(same._gt.seg, det._gt.seg)
    assert torch.equal(same._gt.offsets, det._gt.offsets) and same.dataset_name == "ground_truth"


def test_label_lists_fold_as_in_the_reference(tmp_path):
    path = str(tmp_path / "gt.json")
    with open(path, "w") as f:
        json.dump({"database": {"v": {"subset": "Validation", "annotations": [
            {"segment": [1, 2.5], "label_id": [3, 4]}, {"segment": [0, 1], "label_id": "7"}]}}}, f)
    gt = segmetrics.load_gt_seg_from_json(path, split="validation", label_offset=10)
    assert gt["label"].tolist() == [(10 ** 0 + 4) + (10 ** 1 + 3), 7] and gt["t-end"].tolist() == [2.5, 1.0]
    assert len(segmetrics.load_gt_seg_from_json(path, split="training")["label"]) == 0


def test_remap_drops_labels_absent_from_the_ground_truth():
    gt_labels = torch.tensor([2, 3, 5, 7])
    labels = torch.tensor([5, 0, 2, 1, 7, 100, 3, 4, -1])
    index, keep = segmetrics.remap_labels(labels, gt_labels)
    assert keep.tolist() == [True, False, True, False, True, False, True, False, False]
    assert index[keep].tolist() == [2, 0, 3, 1]
    # the reference's replace() would leave 0 and 1 as they are: the remapped indices of labels 2 and 3 - another class
    ref_index, ref_keep = R.remap(labels.numpy(), gt_labels.numpy())
    assert np.array_equal(ref_index[ref_keep], index[keep].numpy()) and np.array_equal(ref_keep, keep.numpy())


def test_a_class_without_ground_truth_raises():
    empty = {"video-id": [], "t-start": np.zeros(0), "t-end": np.zeros(0)}
    pred = {"video-id": ["a"], "t-start": np.zeros(1), "t-end": np.ones(1), "score": np.ones(1)}
    with pytest.raises(ValueError):
        segmetrics.compute_average_precision_detection(empty, pred)
    with pytest.raises(ValueError):
        R.class_ap([], np.zeros((0, 2)), ["a"], np.array([[0.0, 1.0]]), np.ones(1), [0.5])
    gt = {"video-id": ["a"], "t-start": np.zeros(1), "t-end": np.ones(1)}
    none = {"video-id": [], "t-start": np.zeros(0), "t-end": np.zeros(0), "score": np.zeros(0)}
    assert segmetrics.compute_average_precision_detection(gt, none, np.array([0.3, 0.5])).tolist() == [0.0, 0.0]


def test_results_to_dict_and_array(z):
    results = {"video-id": z["p_vid"].tolist(), "t-start": torch.from_numpy(z["p_t-start"]), "t-end": z["p_t-end"],
               "label": z["p_label"], "score": z["p_score"]}
    d = segmetrics.results_to_dict(results)
    assert list(d) == sorted(set(results["video-id"])) and sum(len(v) for v in d.values()) == len(z["p_score"])
    first = results["video-id"][0]
    assert d[first][0] == {"label": int(z["p_label"][0]), "score": float(z["p_score"][0]),
                           "segment": [float(z["p_t-start"][0]), float(z["p_t-end"][0])]}
    a = segmetrics.results_to_array(results, 10)
    for v, entry in a.items():
        rows = np.where(z["p_vid"] == v)[0]
        rows = rows[np.argsort(-z["p_score"][rows])][:10]
        assert np.array_equal(entry["score"], z["p_score"][rows]) and np.array_equal(entry["label"], z["p_label"][rows])
        assert np.array_equal(entry["segment"], np.stack([z["p_t-start"][rows], z["p_t-end"][rows]], 1))


@pytest.mark.parametrize("num_pred, topk", [(10, 1), (10, 2), (200, 1), (200, 2)])
def test_restatement_reproduces_the_recorded_postprocessing(z, num_pred, topk):
    results = {"video-id": z["p_vid"].tolist(), "t-start": z["p_t-start"], "t-end": z["p_t-end"], "label": z["p_label"],
               "score": z["p_score"]}
    cls = dict(zip(z["p_cls_vids"].tolist(), z["p_cls"]))
    out, tag = R.postprocess(results, cls, num_pred, topk), f"p_n{num_pred}_k{topk}_"
    assert out["video-id"] == z[tag + "vid"].tolist()
    for k in ("t-start", "t-end", "label"):
        assert np.array_equal(out[k], z[tag + k])
    np.testing.assert_allclose(out["score"], z[tag + "score"], rtol=2.0 ** -51, atol=0)
    counts = np.bincount(np.unique(z["p_vid"], return_inverse=True)[1])
    assert counts.min() < 10 < counts.max() < 200                           # num_pred = 10 cuts some videos, 200 none
    assert len(out["score"]) == topk * np.minimum(counts, num_pred).sum()


def test_drop_in_names_keep_the_reference_signatures():
    def names(f):
        return list(inspect.signature(f).parameters)

    assert names(segmetrics.ANETdetection.__init__)[:8] == ["self", "ant_file", "split", "tiou_thresholds", "label", "label_offset",
                                                            "num_workers", "dataset_name"]
    sig = inspect.signature(segmetrics.ANETdetection.__init__).parameters
    assert sig["split"].default is None and sig["label"].default == "label_id" and sig["label_offset"].default == 0
    assert sig["num_workers"].default == 8 and np.array_equal(sig["tiou_thresholds"].default, np.linspace(0.1, 0.5, 5))
    assert sig["ground_truth"].kind is inspect.Parameter.KEYWORD_ONLY
    assert names(segmetrics.ANETdetection.evaluate) == ["self", "preds", "verbose"]
    assert names(segmetrics.compute_average_precision_detection) == ["ground_truth", "prediction", "tiou_thresholds"]
    assert names(segmetrics.load_gt_seg_from_json) == ["json_file", "split", "label", "label_offset"]
    assert names(segmetrics.load_pred_seg_from_json) == ["json_file", "label", "label_offset"]
    assert names(segmetrics.postprocess_results) == ["results", "cls_score_file", "num_pred", "topk"]
    post = inspect.signature(segmetrics.postprocess_results).parameters
    assert post["num_pred"].default == 200 and post["topk"].default == 2
    assert names(segmetrics.results_to_array) == ["results", "num_pred"] and names(segmetrics.results_to_dict) == ["results"]
    source = inspect.getsource(segmetrics)
    assert "import pandas" not in source and "import joblib" not in source


def test_cpu_tensors_raise():
    seg, off = torch.zeros(2, 2, dtype=torch.float64), torch.tensor([0, 2], dtype=torch.int32)
    with pytest.raises(NotImplementedError):
        ops.seg_ap_match(seg, off, seg, off, [0.5])
    with pytest.raises(NotImplementedError):
        ops.seg_ap(torch.zeros(1, 2, dtype=torch.int32), torch.zeros(2, dtype=torch.int32), off, torch.ones(1, dtype=torch.int32))


def test_header_exports_and_argument_checks():
    L = hip.lib()
    for name in ("otp_seg_ap_match", "otp_seg_ap", "otp_seg_ap_match_workspace"):
        assert name in hip.SIGNATURES and hasattr(L, name)
    cap, max_t = hip.CONSTANTS["OTP_SEG_AP_LDS_GT"], hip.CONSTANTS["OTP_SEG_AP_MAX_THRESHOLDS"]
    assert max_t == 32 and cap % 64 == 0 and 2 * 8 * cap <= 64 * 1024         # both ends of the staged segments fit in LDS
    ws = L.otp_seg_ap_match_workspace
    assert ws(0, 10, 5) == 0 and ws(3, 0, 5) == 0 and ws(3, 10, 0) == 0
    assert ws(1, 100000, 5) == ws(4000, 100000, 5) == 5 * ws(7, 100000, 1)  # the groups share the rows, whatever G is
    for m in (1, cap, cap + 1, 5 * cap + 77, 1 << 20):                      # a lock bit for every ground truth, with room to align
        assert 8 * ws(1, m, 1) >= m and ws(1, m, 1) % 4 == 0
    bad, short, unsup = (hip.CONSTANTS[k] for k in ("OTP_ERR_BAD_ARG", "OTP_ERR_WORKSPACE", "OTP_ERR_UNSUPPORTED"))
    p = 64                                                                   # any non-null address: every call below returns first
    thr = (ctypes.c_double * 40)(*([0.5] * 40))
    nan = (ctypes.c_double * 2)(0.5, float("nan"))
    big = 1 << 40
    assert L.otp_seg_ap_match(None, p, p, p, thr, 1, 4, 4, 5, p, big, p, None) == bad
    assert L.otp_seg_ap_match(p, p, p, p, None, 1, 4, 4, 5, p, big, p, None) == bad
    assert L.otp_seg_ap_match(p, p, p, p, thr, 1, 4, 4, 5, p, big, None, None) == bad
    assert L.otp_seg_ap_match(p, p, p, p, thr, 0, 4, 4, 5, p, big, p, None) == bad
    assert L.otp_seg_ap_match(p, p, p, p, thr, 1, 4, 4, 0, p, big, p, None) == bad
    assert L.otp_seg_ap_match(p, p, p, p, nan, 1, 4, 4, 2, p, big, p, None) == bad
    assert L.otp_seg_ap_match(p, p, p, p, thr, 1, 4, 4, max_t + 1, p, big, p, None) == unsup
    assert L.otp_seg_ap_match(p, p, p, p, thr, 1, 1 << 28, 4, 5, p, big, p, None) == unsup
    assert L.otp_seg_ap_match(p, p, p, p, thr, 1, 4, 1 << 28, 5, p, big, p, None) == unsup
    assert L.otp_seg_ap_match(p, p, p, p, thr, 1, 4, 4, 5, p, ws(1, 4, 5) - 1, p, None) == short
    assert L.otp_seg_ap(None, p, p, p, 3, 5, 4, p, None) == bad
    assert L.otp_seg_ap(p, p, p, p, 0, 5, 4, p, None) == bad
    assert L.otp_seg_ap(p, p, p, p, 3, 0, 4, p, None) == bad
    assert L.otp_seg_ap(p, p, p, p, 3, 5, 4, None, None) == bad
    assert L.otp_seg_ap(p, p, p, p, 3, max_t + 1, 4, p, None) == unsup
    assert L.otp_seg_ap(p, p, p, p, 3, 5, 1 << 28, p, None) == unsup
