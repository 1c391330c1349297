#!/usr/bin/env python
"""Generate tests/golden/segap.npz by RUNNING the reference's temporal detection metric (build container only).

Run from the repo root:  ``python tests/golden/make_golden_segap.py``

The reference's ``thirdparty/utils/metrics.py`` and ``postprocessing.py`` are loaded from their files (pandas and joblib are
needed for that; ``np.float = float`` is set in this process first, the one thing the reference needs on numpy 2).  The ground
truth of a case is written to a JSON file in the temporary folder, the reference's ``ANETdetection`` /
``compute_average_precision_detection`` / ``postprocess_results`` run on it, and their results are what is recorded.  On every
case the restatement tests/segap_ref.py is asserted to reproduce the reference's ``ap`` BIT FOR BIT; the ``match`` tables, which
the reference keeps internal, are the restatement's.  If the reference cannot be loaded the restatement alone is the yardstick,
and ``yardstick`` in the file says which it was.

Match-kernel batch ``m``: one flat batch of groups (ground truths, predictions) = GROUPS_M, scored as one class whose videos
are the groups, at T = 1, 5 and 10 thresholds; a further group holds one zero-length prediction on one identical zero-length
ground truth (tIoU = 0 / 0), recorded only if the reference answers it the same way twice and as the restatement does.
AP-kernel case ``a``: eight classes with 0, 1, 255, 256, 257 and 5000 predictions, one whose predictions are all true
positives and one whose predictions are all false positives.  End-to-end case ``e``: 12 videos x 6 classes, one class without
predictions, one video without ground truth, prediction labels outside the ground truth, three videos of another split;
its prediction values are float32 numbers, so that float32 and float64 inputs say the same.  ``p``: ``postprocess_results`` with
topk 1 and 2 and num_pred below and above the videos' counts.

The margins that make every decision well defined are ASSERTED: scores inside a class differ by >= 1e-9; for every prediction
the positive tIoUs to its ground truths differ by >= 1e-9; every tIoU is >= 1e-9 from every threshold; prediction labels
absent from the ground truth do not fall in 0 .. C-1 (so the reference, which leaves them unchanged, and the drop rule agree).
The data of a case comes from one seed; a seed that fails a margin is skipped for the next one (``seeds`` in the file records
the ones used) - the margins never move.
"""
from __future__ import annotations

import importlib.util
import json
import os
import pickle
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import REF, save                             # noqa: E402
from otpose_amd import hip                                    # noqa: E402
from tests import segap_ref as R                              # noqa: E402

CAP = hip.CONSTANTS["OTP_SEG_AP_LDS_GT"]
GROUPS_M = ((0, 5), (1, 0), (1, 1), (2, 7), (63, 200), (64, 200), (65, 200), (CAP + 1, 40), (4, 1025))
THRESHOLDS = {1: np.array([0.5]), 5: np.linspace(0.1, 0.5, 5), 10: np.linspace(0.5, 0.95, 10)}
LIMITS = {"score": 1e-9, "tiou": 1e-9, "thr": 1e-9}
POST_RUNS = ((10, 1), (10, 2), (200, 1), (200, 2))            # (num_pred, topk)


def load_reference():
    """(metrics module, postprocessing module) of the reference, or (None, None)."""
    try:
        import joblib                                         # noqa: F401
        import pandas                                         # noqa: F401
        if not hasattr(np, "float"):
            np.float = float                                  # metrics.py:273-274
        pkg = types.ModuleType("reference_utils")
        pkg.__path__ = []
        sys.modules["reference_utils"] = pkg
        mods = []
        for name in ("metrics", "postprocessing"):
            spec = importlib.util.spec_from_file_location("reference_utils." + name,
                                                          os.path.join(REF, "thirdparty", "utils", name + ".py"))
            mod = importlib.util.module_from_spec(spec)
            sys.modules[spec.name] = mod
            spec.loader.exec_module(mod)
            mods.append(mod)
        return tuple(mods)
    except Exception as e:                                    # no pandas, no joblib: the restatement is the yardstick
        print("reference not loaded:", e)
        return None, None


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def margins_ok(m):
    return all(m.get(k, np.inf) >= v for k, v in LIMITS.items())


def search(build, first_seed, what):
    for seed in range(first_seed, first_seed + 200):
        m = {}
        res = build(seed, m)
        if margins_ok(m):
            print(f"{what}: seed {seed}, margins", {k: float(f"{v:.3g}") for k, v in m.items()})
            return seed, res
    raise AssertionError(f"{what}: no seed in 200 keeps the margins")


def timeline(rs, m):
    """m ground-truth segments along a line, neighbours overlapping now and then."""
    start = np.cumsum(rs.uniform(3, 10, m))
    return np.stack([start, start + rs.uniform(2, 12, m)], 1)


def around(rs, gt, n, far=0.15):
    """n predictions: jittered copies of random ground truths, a share of them far from all."""
    if len(gt) == 0:
        s = rs.uniform(0, 100, n)
        return np.stack([s, s + rs.uniform(1, 10, n)], 1)
    pick = gt[rs.randint(0, len(gt), n)]
    length = (pick[:, 1] - pick[:, 0])[:, None]
    seg = pick + rs.uniform(-0.45, 0.45, (n, 2)) * length
    away = rs.uniform(0, 1, n) < far
    seg[away] += gt[:, 1].max() + 50
    return seg


def distinct_scores(rs, n, lo=0.02, hi=0.99):
    return (np.linspace(lo, hi, n) + rs.uniform(-0.3, 0.3, n) * (hi - lo) / max(n, 1))[rs.permutation(n)]


def frame(pd, table):
    return pd.DataFrame({k: (list(v) if k == "video-id" else v) for k, v in table.items()})


def gt_json(path, gt, subsets=None, extra_videos=()):
    db = {}
    for v, s, e, l in zip(gt["video-id"], gt["t-start"], gt["t-end"], gt["label"]):
        db.setdefault(v, {"subset": (subsets or {}).get(v, "validation"), "annotations": []})
        db[v]["annotations"].append({"segment": [float(s), float(e)], "label_id": int(l)})
    for v in extra_videos:
        db[v] = {"subset": "validation", "annotations": []}
    text = json.dumps({"database": db})
    with open(path, "w") as f:
        f.write(text)
    return text


# ---- the match-kernel batch ------------------------------------------------------------------------------------------------
def build_match_batch(seed, margins, with_nan):
    rs = np.random.RandomState(seed)
    groups = [(timeline(rs, m), m, n) for m, n in GROUPS_M]
    total = sum(n for _, _, n in groups) + (1 if with_nan else 0)
    scores = distinct_scores(rs, total)
    gt_l, pred_l, score_l, at = [], [], [], 0
    for gt, m, n in groups:
        pred, sc = around(rs, gt, n), scores[at:at + n]
        at += n
        by = np.argsort(-sc, kind="stable")                    # the kernel takes a group in descending score
        gt_l.append(gt)
        pred_l.append(pred[by])
        score_l.append(sc[by])
    if with_nan:
        gt_l.append(np.array([[7.0, 7.0]]))
        pred_l.append(np.array([[7.0, 7.0]]))
        score_l.append(scores[at:at + 1])
    out = dict(gt_seg=np.concatenate(gt_l), pred_seg=np.concatenate(pred_l), score=np.concatenate(score_l),
               gt_offsets=np.concatenate([[0], np.cumsum([len(g) for g in gt_l])]).astype(np.int32),
               pred_offsets=np.concatenate([[0], np.cumsum([len(p) for p in pred_l])]).astype(np.int32))
    for T, thr in THRESHOLDS.items():
        out[f"match_T{T}"] = R.match_groups(out["pred_seg"], out["pred_offsets"], out["gt_seg"], out["gt_offsets"], thr, margins)
    R._note(margins, "score", np.diff(np.sort(out["score"])).min())
    return out


def match_batch_as_class(b):
    """The batch as one class: group g is video 'g<g>'."""
    gv = np.repeat(np.arange(len(b["gt_offsets"]) - 1), np.diff(b["gt_offsets"]))
    pv = np.repeat(np.arange(len(b["pred_offsets"]) - 1), np.diff(b["pred_offsets"]))
    gt = {"video-id": [f"g{g}" for g in gv], "t-start": b["gt_seg"][:, 0], "t-end": b["gt_seg"][:, 1]}
    pred = {"video-id": [f"g{g}" for g in pv], "t-start": b["pred_seg"][:, 0], "t-end": b["pred_seg"][:, 1], "score": b["score"]}
    return gt, pred


def check_match_batch(b, metrics):
    """The restatement's AP of the batch at every T; equal to its match tables' and, with the reference, to the reference's."""
    gt, pred = match_batch_as_class(b)
    aps = {}
    for T, thr in THRESHOLDS.items():
        ap, match, tp, order = R.class_ap(np.array(gt["video-id"], dtype=object), b["gt_seg"], np.array(pred["video-id"], dtype=object),
                                          b["pred_seg"], b["score"], thr)
        assert np.array_equal(match, b[f"match_T{T}"][:, order])            # both ways round to the same assignment
        if metrics is not None:
            import pandas as pd
            ref = metrics.compute_average_precision_detection(frame(pd, gt), frame(pd, pred), thr)
            assert same(ref, ap), (T, ref, ap)
            ap = ref
        aps[T] = ap
    return aps


# ---- the AP-kernel case ----------------------------------------------------------------------------------------------------
def build_ap_case(seed, margins):
    rs = np.random.RandomState(seed)
    counts = {0: 0, 1: 1, 2: 255, 3: 256, 4: 257, 5: 5000}
    videos = [f"v{i:02d}" for i in range(40)]
    gt = {"video-id": [], "t-start": [], "t-end": [], "label": []}
    preds = {"video-id": [], "t-start": [], "t-end": [], "label": [], "score": []}

    def add(table, vid, seg, label, score=None):
        table["video-id"] += [vid] * len(seg)
        table["t-start"] += seg[:, 0].tolist()
        table["t-end"] += seg[:, 1].tolist()
        table["label"] += [label] * len(seg)
        if score is not None:
            table["score"] += score.tolist()

    for c, n in counts.items():
        per_video = {v: timeline(rs, rs.randint(1, 11) if c == 5 else rs.randint(1, 4)) for v in videos[:30]}
        for v, g in per_video.items():
            add(gt, v, g, 10 + c)
        sc, at = distinct_scores(rs, n), 0
        share = rs.multinomial(n, np.ones(30) / 30)              # the last two of these videos have no ground truth at all
        for v, k in zip(videos[:28] + videos[38:], share):
            add(preds, v, around(rs, per_video.get(v, np.zeros((0, 2))), k), 10 + c, sc[at:at + k])
            at += k
    # class 6: every prediction is a ground truth itself (disjoint inside a video); class 7: every prediction misses
    sc6, sc7 = distinct_scores(rs, 30), distinct_scores(rs, 20)
    for i, v in enumerate(videos[:10]):
        start = np.arange(3) * 40.0 + rs.uniform(0, 5, 3)
        g = np.stack([start, start + rs.uniform(5, 20, 3)], 1)
        add(gt, v, g, 16)
        add(preds, v, g, 16, sc6[3 * i:3 * i + 3])
        add(gt, v, g + 1000, 17)
        add(preds, v, g[:2] + 5000, 17, sc7[2 * i:2 * i + 2])
    gt = {k: (v if k == "video-id" else np.array(v)) for k, v in gt.items()}
    preds = {k: (v if k == "video-id" else np.array(v)) for k, v in preds.items()}
    thr = THRESHOLDS[5]
    return gt, preds, R.kernel_tables(gt, preds, thr, margins), R.detection_ap(gt, preds, thr, margins)[0]


# ---- the end-to-end case ---------------------------------------------------------------------------------------------------
E_LABELS = (2, 3, 5, 7, 11, 13)


def build_e2e_case(seed, margins):
    rs = np.random.RandomState(seed)
    videos = [f"video_{i:02d}" for i in range(12)]
    subsets = {v: ("training" if i >= 9 else "validation") for i, v in enumerate(videos)}
    gt = {"video-id": [], "t-start": [], "t-end": [], "label": []}
    preds = {"video-id": [], "t-start": [], "t-end": [], "label": [], "score": []}
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)   # noqa: E731
    for v in videos:
        for label in E_LABELS:
            g = timeline(rs, rs.randint(0, 5))
            if v != "video_08":                                   # a video of the split without ground truth
                gt["video-id"] += [v] * len(g)
                gt["t-start"] += g[:, 0].tolist()
                gt["t-end"] += g[:, 1].tolist()
                gt["label"] += [label] * len(g)
            if label == 7:                                        # a class without predictions
                continue
            p = f32(around(rs, g, rs.randint(2, 12)))
            for lab, rows in ((label, p), (100 + label % 2, p[:2])):   # labels 100, 101: not in the ground truth
                preds["video-id"] += [v] * len(rows)
                preds["t-start"] += rows[:, 0].tolist()
                preds["t-end"] += rows[:, 1].tolist()
                preds["label"] += [lab] * len(rows)
    preds["score"] = f32(distinct_scores(rs, len(preds["label"])))
    gt = {k: (v if k == "video-id" else np.array(v)) for k, v in gt.items()}
    preds = {k: (v if k == "video-id" else np.array(v)) for k, v in preds.items()}
    in_split = np.array([subsets[v] == "validation" for v in gt["video-id"]])
    gt_split = {k: ([x for x, s in zip(v, in_split) if s] if k == "video-id" else v[in_split]) for k, v in gt.items()}
    C = len(np.unique(gt_split["label"]))
    assert C == len(E_LABELS) and not np.isin(preds["label"][~np.isin(preds["label"], E_LABELS)], np.arange(C)).any()
    # scores only have to differ inside a class: class_ap notes that margin
    ap, _, _ = R.detection_ap(gt_split, preds, THRESHOLDS[5], margins)
    ap10, _, _ = R.detection_ap(gt_split, preds, THRESHOLDS[10], margins)
    return gt, subsets, preds, ap, ap10


# ---- postprocess_results ---------------------------------------------------------------------------------------------------
def build_post_case(seed):
    rs = np.random.RandomState(seed)
    vids = ["c", "a", "e", "b", "d"]
    counts = [3, 10, 11, 30, 7]
    results = {"video-id": [], "t-start": [], "t-end": [], "label": [], "score": []}
    for v, n in zip(vids, counts):
        s = rs.uniform(0, 100, n)
        results["video-id"] += [v] * n
        results["t-start"] += s.tolist()
        results["t-end"] += (s + rs.uniform(1, 20, n)).tolist()
        results["label"] += rs.randint(0, 10, n).tolist()
    results["score"] = distinct_scores(rs, len(results["label"]))
    order = rs.permutation(len(results["label"]))                 # the rows of a video are not contiguous
    results = {k: ([v[i] for i in order] if k == "video-id" else np.array(v)[order]) for k, v in results.items()}
    cls = {v: distinct_scores(rs, 10, 0.01, 0.9) for v in vids}
    return results, cls


def main():
    metrics, post = load_reference()
    out, seeds = {}, {}
    out["yardstick"] = np.array("reference" if metrics is not None else "restatement")
    tmp = tempfile.mkdtemp(prefix="otpose_segap_")

    # match-kernel batch
    seed, b = search(lambda s, m: build_match_batch(s, m, True), 100, "match batch with the 0 / 0 group")
    nan_ok = False
    try:                                                          # the reference's answer to 0 / 0, twice, and the restatement's
        aps, again = check_match_batch(b, metrics), check_match_batch(b, metrics)
        nan_ok = all(same(aps[T], again[T]) for T in THRESHOLDS) and all((b[f"match_T{T}"][:, -1] == 0).all() for T in THRESHOLDS)
    except Exception as e:
        print("the 0 / 0 group is not recorded:", repr(e))
    if not nan_ok:
        seed, b = search(lambda s, m: build_match_batch(s, m, False), 100, "match batch")
        aps = check_match_batch(b, metrics)
    print("0 / 0 group recorded:", nan_ok)
    seeds["m"] = seed
    out["m_nan_group"] = np.array(nan_ok)
    for k, v in b.items():
        out["m_" + k] = v
    for T in THRESHOLDS:
        out[f"m_ap_T{T}"] = aps[T]
        out[f"thresholds_T{T}"] = THRESHOLDS[T]

    # AP-kernel case
    seed, (gt, preds, tables, ap) = search(build_ap_case, 200, "ap case")
    seeds["a"] = seed
    assert same(tables["ap"], ap)
    if metrics is not None:
        import pandas as pd
        path = os.path.join(tmp, "a.json")
        gt_json(path, gt)
        det = metrics.ANETdetection(path, split="validation", tiou_thresholds=THRESHOLDS[5], num_workers=1)
        det.evaluate(frame(pd, preds), verbose=False)
        assert same(det.ap, ap), np.abs(det.ap - ap).max()
        ap = det.ap
    sizes = np.diff(tables["class_offsets"]).tolist()
    assert sizes[:6] == [0, 1, 255, 256, 257, 5000] and sizes[6:] == [30, 20], sizes
    tp = [(tables["match"][:, tables["order"][tables["class_offsets"][c]:tables["class_offsets"][c + 1]]] >= 0) for c in (6, 7)]
    assert tp[0].all() and not tp[1].any()
    for k in ("match", "order", "class_offsets", "npos"):
        out["a_" + k] = tables[k]
    out["a_ap"] = ap

    # end-to-end case
    seed, (gt, subsets, preds, ap, ap10) = search(build_e2e_case, 300, "e2e case")
    seeds["e"] = seed
    path = os.path.join(tmp, "e.json")
    out["e_gt_json"] = np.array(gt_json(path, gt, subsets, extra_videos=("video_08",)))
    if metrics is not None:
        import pandas as pd
        for thr, mine, tag in ((THRESHOLDS[5], ap, "ap"), (THRESHOLDS[10], ap10, "ap10")):
            det = metrics.ANETdetection(path, split="validation", tiou_thresholds=thr, num_workers=1)
            mAP, avg = det.evaluate(frame(pd, preds), verbose=False)
            assert same(det.ap, mine), (tag, np.abs(det.ap - mine).max())
            assert det.activity_index == {l: i for i, l in enumerate(E_LABELS)}
        ap, ap10 = (ap, ap10)
    out["e_ap"], out["e_ap10"] = ap, ap10
    out["e_pred_vid"] = np.array(preds["video-id"])
    for k in ("t-start", "t-end", "label", "score"):
        out["e_pred_" + k] = preds[k]
    # one class through compute_average_precision_detection: label 5 of the split's ground truth
    out["e_labels"] = np.array(E_LABELS)

    # postprocess_results
    results, cls = build_post_case(400)
    seeds["p"] = 400
    out["p_vid"] = np.array(results["video-id"])
    for k in ("t-start", "t-end", "label", "score"):
        out["p_" + k] = results[k]
    out["p_cls_vids"] = np.array(sorted(cls))
    out["p_cls"] = np.stack([cls[v] for v in sorted(cls)])
    for num_pred, topk in POST_RUNS:
        mine = R.postprocess(results, cls, num_pred, topk)
        if post is not None:
            cls_path = os.path.join(tmp, "cls.pkl")
            with open(cls_path, "wb") as f:
                pickle.dump(cls, f)
            ref = post.postprocess_results(dict(results), cls_path, num_pred=num_pred, topk=topk)
            assert ref["video-id"] == mine["video-id"]
            for k in ("t-start", "t-end", "label"):
                assert np.array_equal(ref[k], mine[k]), k
            assert np.allclose(ref["score"], mine["score"], rtol=2.0 ** -51, atol=0)
            mine = ref
        tag = f"p_n{num_pred}_k{topk}_"
        out[tag + "vid"] = np.array(mine["video-id"])
        for k in ("t-start", "t-end", "label", "score"):
            out[tag + k] = np.asarray(mine[k])

    out["seeds"] = np.array(repr(sorted(seeds.items())))
    out["limits"] = np.array(repr(sorted(LIMITS.items())))
    save("segap", **out)


if __name__ == "__main__":
    main()
