"""Temporal detection mAP on the GPU (csrc/segap.hip, otpose_amd/segmetrics.py) against the recorded results of the reference
(tests/golden/segap.npz): each kernel through the C ABI's Python wrapper and each drop-in name.

Matches are compared exactly.  AP is compared within 4 (K + 2) 2^-53, K the true positives of that (class, threshold): the
kernel's terms are bitwise the reference's (the same correctly rounded float64 quotients and products); only the order in
which at most K + 2 terms, all within [0, 1], are added differs, and every partial sum is at most 1.  The bound is derived,
not tuned; the largest deviation seen is printed (DESIGN.md section 3.15 records it).

``postprocess_results``: labels and segments are copies; a score is sqrt of a product that rounds identically on both sides,
and each side's square root is within one ulp: 2^-51 relative.
"""
import json
import os
import pickle

import numpy as np
import pytest
import torch

from otpose_amd import hip, ops, segmetrics, segnms
from tests import segap_ref as R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "segap.npz")
_worst = {"ap": 0.0}


@pytest.fixture(scope="module")
def z():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope="module")
def gt_json(z, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("segap") / "e2e.json")
    with open(path, "w") as f:
        f.write(str(z["e_gt_json"]))
    return path


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def check_ap(got, want, true_positives):
    """|got - want| <= 4 (K + 2) 2^-53 entry by entry; prints the largest deviation."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape == np.shape(true_positives) and got.dtype == np.float64
    d = np.abs(got - want)
    _worst["ap"] = max(_worst["ap"], float(d.max()))
    print(f"ap: largest deviation {d.max():.3e} = {d.max() * 2.0 ** 53:.2f} x 2^-53 (worst so far {_worst['ap']:.3e})")
    assert (d <= 4.0 * (np.asarray(true_positives) + 2) * 2.0 ** -53).all()


def true_positives(match, order, class_offsets):
    """(T, C) true positives of a match table."""
    return np.stack([(match[:, order[class_offsets[c]:class_offsets[c + 1]]] >= 0).sum(axis=1)
                     for c in range(len(class_offsets) - 1)], 1)


def e2e_preds(z):
    return {"video-id": z["e_pred_vid"].tolist(), "t-start": z["e_pred_t-start"], "t-end": z["e_pred_t-end"],
            "label": z["e_pred_label"], "score": z["e_pred_score"]}


def e2e_tables(gt_json, z, T):
    return R.kernel_tables(segmetrics.load_gt_seg_from_json(gt_json, split="validation"), e2e_preds(z), z[f"thresholds_T{T}"])


@pytest.mark.parametrize("T", [1, 5, 10])
def test_match_kernel(z, T):
    match = ops.seg_ap_match(dev(z["m_pred_seg"]), dev(z["m_pred_offsets"]), dev(z["m_gt_seg"]), dev(z["m_gt_offsets"]),
                             z[f"thresholds_T{T}"])
    assert match.dtype == torch.int32 and match.is_cuda
    assert np.array_equal(match.cpu().numpy(), z[f"m_match_T{T}"])
    sizes = np.diff(z["m_gt_offsets"])
    assert sizes.max() > hip.CONSTANTS["OTP_SEG_AP_LDS_GT"] >= 65                # the LDS and the workspace path both ran


def test_match_kernel_on_groups_with_more_than_one_lock_word_per_lane():
    """Two neighbouring workspace groups, the first with more than 2048 ground truths (a lane then owns more than 32 of them),
    against the restatement; the margins of the golden file are asserted here too."""
    rs = np.random.RandomState(7)
    thr = np.linspace(0.1, 0.5, 5)
    gts, preds = [], []
    for m, n in ((2100, 30), (1500, 20), (3, 4)):
        start = np.cumsum(rs.uniform(3, 10, m))
        gt = np.stack([start, start + rs.uniform(2, 12, m)], 1)
        pick = gt[rs.randint(0, m, n)]
        preds.append(pick + rs.uniform(-0.45, 0.45, (n, 2)) * (pick[:, 1] - pick[:, 0])[:, None])
        gts.append(gt)
    gt_seg, pred_seg = np.concatenate(gts), np.concatenate(preds)
    gt_off = np.concatenate([[0], np.cumsum([len(g) for g in gts])]).astype(np.int32)
    pred_off = np.concatenate([[0], np.cumsum([len(p) for p in preds])]).astype(np.int32)
    margins = {}
    want = R.match_groups(pred_seg, pred_off, gt_seg, gt_off, thr, margins)
    assert margins["tiou"] >= 1e-9 and margins["thr"] >= 1e-9 and (want >= 0).sum() > 100
    got = ops.seg_ap_match(dev(pred_seg), dev(pred_off), dev(gt_seg), dev(gt_off), thr)
    assert np.array_equal(got.cpu().numpy(), want)


def test_a_group_outside_the_batch_is_answered_with_minus_one(z):
    o0, o1 = int(z["m_pred_offsets"][3]), int(z["m_pred_offsets"][4])            # the group with 2 ground truths and 7 predictions
    q0, q1 = int(z["m_gt_offsets"][3]), int(z["m_gt_offsets"][4])
    pred, gt = dev(z["m_pred_seg"][o0:o1]), dev(z["m_gt_seg"][q0:q1])
    thr = z["thresholds_T5"]
    want = z["m_match_T5"][:, o0:o1]
    assert (want >= 0).any()

    def run(pred_off, gt_off):
        return ops.seg_ap_match(pred, torch.tensor(pred_off, dtype=torch.int32, device="cuda"), gt,
                                torch.tensor(gt_off, dtype=torch.int32, device="cuda"), thr).cpu().numpy()

    assert np.array_equal(run([0, 7], [0, 2]), want)
    assert (run([0, 7], [0, 3]) == -1).all() and (run([0, 7], [2, 0]) == -1).all()      # ground truths past the rows, backwards
    assert (run([0, 8], [0, 2]) == -1).all() and (run([-1, 7], [0, 2]) == -1).all()     # predictions that cannot be named
    got = run([0, 3, 3], [0, 0, 2])                                                       # rows 3 .. 6 belong to no group
    assert (got == -1).all()
    assert np.array_equal(run([0, 0, 7], [0, 0, 2]), want)                               # an empty group in front


def test_ap_kernel(z):
    ap = ops.seg_ap(dev(z["a_match"]), dev(z["a_order"]), dev(z["a_class_offsets"]), dev(z["a_npos"]))
    assert ap.is_cuda and ap.dtype == torch.float64
    ap = ap.cpu().numpy()
    check_ap(ap, z["a_ap"], true_positives(z["a_match"], z["a_order"], z["a_class_offsets"]))
    assert (ap[:, 0] == 0).all() and (ap[:, 6] == 1).all() and (ap[:, 7] == 0).all()   # no predictions, all true, all false


@pytest.mark.parametrize("T, key", [(5, "e_ap"), (10, "e_ap10")])
def test_evaluate_end_to_end(z, gt_json, capsys, T, key):
    thr = z[f"thresholds_T{T}"]
    det = segmetrics.ANETdetection(gt_json, split="validation", tiou_thresholds=thr)
    mAP, average = det.evaluate(e2e_preds(z), verbose=True)
    tables = e2e_tables(gt_json, z, T)
    with capsys.disabled():
        check_ap(det.ap, z[key], true_positives(tables["match"], tables["order"], tables["class_offsets"]))
    assert np.array_equal(mAP, det.ap.mean(axis=1)) and average == mAP.mean() and isinstance(mAP, np.ndarray)
    printed = capsys.readouterr().out
    assert "[RESULTS] Action detection results on e2e." in printed and f"|tIoU = {thr[0]:.2f}: mAP = {mAP[0] * 100:.2f} (%)" in printed
    assert det.activity_index == {int(l): i for i, l in enumerate(z["e_labels"])}


def test_every_input_form_gives_the_same_bytes(z, gt_json, tmp_path):
    det = segmetrics.ANETdetection(gt_json, split="validation")
    preds = e2e_preds(z)
    det.evaluate(preds, verbose=False)
    want = det.ap.tobytes()

    class Columns:                                              # anything indexable by column name, as a data frame is
        def __init__(self, table):
            self.table = table

        def __getitem__(self, name):
            return self.table[name]

        def __len__(self):
            return len(self.table["score"])

    f32 = {k: (v if k == "video-id" else dev(v.astype(np.int64 if k == "label" else np.float32))) for k, v in preds.items()}
    assert all(np.array_equal(f32[k].cpu().numpy().astype(np.float64), preds[k]) for k in ("t-start", "t-end", "score"))
    cpu = {k: (v if k == "video-id" else torch.from_numpy(v)) for k, v in preds.items()}
    path = str(tmp_path / "pred.json")
    db = {}
    for v, s, e, l, p in zip(preds["video-id"], preds["t-start"], preds["t-end"], preds["label"], preds["score"]):
        db.setdefault(v, []).append({"segment": [float(s), float(e)], "label_id": int(l), "scores": float(p)})
    with open(path, "w") as f:
        json.dump({"database": db}, f)
    for form in (f32, cpu, Columns(preds), path):
        det.evaluate(form, verbose=False)
        assert det.ap.tobytes() == want
    from_table = segmetrics.ANETdetection(None, ground_truth=segmetrics.load_gt_seg_from_json(gt_json, split="validation"))
    from_table.evaluate(f32, verbose=False)
    assert from_table.ap.tobytes() == want


def test_compute_average_precision_detection_on_one_class(z, gt_json):
    gt, preds = segmetrics.load_gt_seg_from_json(gt_json, split="validation"), e2e_preds(z)
    label, c = 5, 2
    assert z["e_labels"][c] == label
    g, p = gt["label"] == label, preds["label"] == label
    one_gt = {k: v[g] for k, v in gt.items()}
    one_pred = {k: (np.asarray(v, dtype=object)[p] if k == "video-id" else dev(v[p])) for k, v in preds.items()}
    thr = z["thresholds_T5"]
    ap = segmetrics.compute_average_precision_detection(one_gt, one_pred, thr)
    tables = e2e_tables(gt_json, z, 5)
    k = true_positives(tables["match"], tables["order"], tables["class_offsets"])[:, c]
    check_ap(ap, z["e_ap"][:, c], k)


@pytest.mark.parametrize("num_pred, topk", [(10, 1), (10, 2), (200, 1), (200, 2)])
def test_postprocess_results(z, tmp_path, num_pred, topk):
    results = {"video-id": z["p_vid"].tolist(), "t-start": dev(z["p_t-start"]), "t-end": dev(z["p_t-end"]),
               "label": dev(z["p_label"]), "score": dev(z["p_score"])}
    cls = dict(zip(z["p_cls_vids"].tolist(), z["p_cls"]))
    pkl, js = str(tmp_path / "cls.pkl"), str(tmp_path / "cls.json")
    with open(pkl, "wb") as f:
        pickle.dump(cls, f)
    with open(js, "w") as f:
        json.dump({"results": {k: v.tolist() for k, v in cls.items()}}, f)
    tag = f"p_n{num_pred}_k{topk}_"
    outs = [segmetrics.postprocess_results(results, source, num_pred=num_pred, topk=topk) for source in (cls, pkl, js)]
    for out in outs:
        assert out["video-id"] == z[tag + "vid"].tolist()
        assert all(out[k].is_cuda for k in ("t-start", "t-end", "label", "score"))
        for k in ("t-start", "t-end", "label"):
            assert np.array_equal(out[k].cpu().numpy(), z[tag + k])
        score, want = out["score"].cpu().numpy(), z[tag + "score"]
        assert score.dtype == np.float64 and (np.abs(score - want) <= 2.0 ** -51 * np.abs(want)).all()
        assert out["score"].cpu().numpy().tobytes() == outs[0]["score"].cpu().numpy().tobytes()


def test_chain_from_segment_nms_to_map():
    """batched_nms_videos on the three-video batch of segnms.npz; its output goes to evaluate() as device tensors.  The ground
    truth is drawn around every third kept segment.  The yardstick is the restatement on the same NMS output copied to the host."""
    s = dict(np.load(os.path.join(HERE, "golden", "segnms.npz")))
    names = ("mc1", "mc3", "mc20")
    videos = [tuple(dev(s[f"py_{n}_in_{k}"]) for k in ("segs", "scores", "cls")) for n in names]
    kept = segnms.batched_nms_videos(videos, 0.5, 0.001, 100)
    preds = {"video-id": [n for n, (segs, _, _) in zip(names, kept) for _ in range(segs.shape[0])],
             "t-start": torch.cat([k[0][:, 0] for k in kept]), "t-end": torch.cat([k[0][:, 1] for k in kept]),
             "label": torch.cat([k[2] for k in kept]), "score": torch.cat([k[1] for k in kept])}
    assert all(preds[k].is_cuda for k in ("t-start", "t-end", "label", "score")) and preds["score"].dtype == torch.float32
    host = {k: (v if k == "video-id" else v.cpu().numpy()) for k, v in preds.items()}
    rs = np.random.RandomState(3)
    rows = np.arange(0, len(host["score"]), 3)
    length = host["t-end"][rows].astype(np.float64) - host["t-start"][rows]
    gt = {"video-id": [host["video-id"][r] for r in rows],
          "t-start": host["t-start"][rows] + rs.uniform(-0.2, 0.2, len(rows)) * length,
          "t-end": host["t-end"][rows] + rs.uniform(-0.2, 0.2, len(rows)) * length, "label": host["label"][rows]}
    thr = np.linspace(0.3, 0.7, 5)
    margins = {}
    tables = R.kernel_tables(gt, host, thr, margins)
    want, want_mAP, want_avg = R.detection_ap(gt, host, thr, margins)
    assert margins["score"] > 0 and margins["thr"] >= 1e-9 and margins.get("tiou", 1.0) >= 1e-9
    det = segmetrics.ANETdetection(None, tiou_thresholds=thr, ground_truth=gt, dataset_name="chain")
    mAP, avg = det.evaluate(preds, verbose=False)
    k = true_positives(tables["match"], tables["order"], tables["class_offsets"])
    assert k.sum() > 20 and 0 < want_avg < 1
    check_ap(det.ap, want, k)
    assert np.array_equal(mAP, det.ap.mean(axis=1)) and avg == mAP.mean()


def test_two_runs_are_bit_identical(z, gt_json):
    def run():
        match = ops.seg_ap_match(dev(z["m_pred_seg"]), dev(z["m_pred_offsets"]), dev(z["m_gt_seg"]), dev(z["m_gt_offsets"]),
                                 z["thresholds_T10"])
        ap = ops.seg_ap(dev(z["a_match"]), dev(z["a_order"]), dev(z["a_class_offsets"]), dev(z["a_npos"]))
        det = segmetrics.ANETdetection(gt_json, split="validation")
        det.evaluate(e2e_preds(z), verbose=False)
        return match.cpu().numpy().tobytes(), ap.cpu().numpy().tobytes(), det.ap.tobytes()

    assert run() == run()


def test_cpu_tensors_raise(z):
    seg, off = torch.zeros(2, 2, dtype=torch.float64), torch.tensor([0, 2], dtype=torch.int32)
    with pytest.raises(NotImplementedError):
        ops.seg_ap_match(seg, off, seg, off, [0.5])
    with pytest.raises(NotImplementedError):
        ops.seg_ap_match(seg.cuda(), off.cuda(), seg, off.cuda(), [0.5])
    with pytest.raises(ValueError):                             # float32 segments are the caller's to widen
        ops.seg_ap_match(seg.cuda().float(), off.cuda(), seg.cuda(), off.cuda(), [0.5])
