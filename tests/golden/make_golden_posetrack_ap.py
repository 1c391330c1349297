#!/usr/bin/env python
"""Generate tests/golden/posetrack_ap.npz by IMPORTING the reference's PoseTrack evaluator (build container only).

Run from the repo root:  ``python tests/golden/make_golden_posetrack_ap.py``  (writes the same bytes every time).

The reference is imported with ``make_golden.import_reference`` plus empty stand-ins for the modules that are missing on
the build machine (``motmetrics``, ``shapely``, ``yacs``, ``tensorboardX``, ``pycocotools``, next to ``cv2`` /
``torchvision``).  REAL SHAPELY WAS NOT AVAILABLE: ``shapely.geometry.Point`` / ``Polygon.contains`` are replaced by the
float64 even-odd crossing test below, so the vectors pin the reference's evaluator around the polygon test, not shapely's
own predicate; condition (c) keeps every point away from the edges, where the two could differ.

Seeded synthetic input (``otpose_amd.synthetic.posetrack_eval_case``): predictions float32 (N,17,3) + box scores become
prediction frames by the reference's own ``convert_data_to_annorect_struct`` (fed as PoseTrackDataset.evaluate feeds it);
then ``cleanupData``, ``removeIgnoredPoints``, ``assignGTmulti``, ``compute_metrics`` and ``getCum`` of utils/evaluate.py
run.  The conditions under which the reference alone is unambiguous are ASSERTED (the seed must satisfy them); they
exclude nothing from a comparison.
"""
from __future__ import annotations

import copy
import io
import os
import sys
import types
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

from make_golden import import_reference          # noqa: E402
from otpose_amd import synthetic as S             # noqa: E402
import posetrack_ap_ref as R                      # noqa: E402

SEED, FRAMES = 20260117, 60
J = 15


class _Point:
    def __init__(self, x, y):
        self.x, self.y = float(x), float(y)


class _Polygon:
    """Stand-in for shapely.geometry.Polygon: ``contains`` is the even-odd crossing test in float64."""

    def __init__(self, xy):
        self.xy = [(float(x), float(y)) for x, y in xy]

    def contains(self, pt):
        inside = False
        n = len(self.xy)
        for i in range(n):
            xi, yi = self.xy[i]
            xj, yj = self.xy[i - 1]
            if (yi > pt.y) != (yj > pt.y):
                if pt.x < (xj - xi) * (pt.y - yi) / (yj - yi) + xi:
                    inside = not inside
        return inside


def import_evaluator():
    for name in ("motmetrics", "shapely", "shapely.geometry", "yacs", "yacs.config", "tensorboardX", "pycocotools",
                 "pycocotools.coco", "pycocotools.cocoeval", "pycocotools.mask"):
        sys.modules.setdefault(name, types.ModuleType(name))
    geometry = sys.modules["shapely.geometry"]
    geometry.Point, geometry.Polygon = _Point, _Polygon
    sys.modules["shapely"].geometry = geometry
    sys.modules["yacs.config"].CfgNode = dict
    sys.modules["yacs"].config = sys.modules["yacs.config"]
    sys.modules["tensorboardX"].SummaryWriter = object
    import_reference()
    import utils.evaluate as E
    return E


def save_deterministic(path, arrays):
    """An .npz (deflate) with fixed member timestamps: the same arrays give the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            a = np.asarray(arrays[name])
            np.lib.format.write_array(buf, np.ascontiguousarray(a).reshape(a.shape), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    E = import_evaluator()
    gt_frames, preds, box, frame_id = S.posetrack_eval_case(FRAMES, SEED)

    # ---- prediction frames, as dataset/PoseTrackDataset.py:495-505, 560-577 builds them ---------------------------
    pr_frames = []
    for f in range(FRAMES):
        kps, bbs = [], []
        for s in np.nonzero(frame_id == f)[0]:
            temp = np.zeros((4, 17))
            temp[0, :], temp[1, :], temp[2, :], temp[3, :] = preds[s, :, 0], preds[s, :, 1], preds[s, :, 2], preds[s, :, 2]
            kps.append(temp)
            b = np.zeros((1, 6))
            b[0, 5] = box[s]
            bbs.append(b)
        pr_frames.append({"annorect": E.convert_data_to_annorect_struct(kps, list(range(len(kps))), bbs)})

    # the frames "the reference wrote", as arrays (a placeholder person has one point)
    ann_off, ann_pts, ann_xy, ann_score, ann_rect_score, ann_track = [0], [], [], [], [], []
    for fr in pr_frames:
        for rect in fr["annorect"]:
            pts = rect["annopoints"][0]["point"]
            assert [p["id"][0] for p in pts] == list(range(len(pts)))
            xy, sc = np.zeros((J, 2)), np.zeros(J)
            for p in pts:
                xy[p["id"][0]] = (p["x"][0], p["y"][0])
                sc[p["id"][0]] = p["score"][0]
            ann_pts.append(len(pts)), ann_xy.append(xy), ann_score.append(sc)
            ann_rect_score.append(float(rect["score"][0])), ann_track.append(rect["track_id"][0])
        ann_off.append(len(ann_pts))

    # ---- the reference's evaluation ---------------------------------------------------------------------------------
    gt, pr = E.cleanupData(copy.deepcopy(gt_frames), copy.deepcopy(pr_frames))
    kept = [f for f in range(FRAMES) if len(gt_frames[f]["annorect"]) > 0]
    assert len(kept) == len(gt) < FRAMES, "no frame dropped by cleanupData"

    # the packed ground truth, straight from the cleaned frames
    gt_off, poly_off, vert_off, gt_xy, gt_has, gt_head, vert_xy = [0], [0], [0], [], [], [], []
    for fr in gt:
        for rect in fr["annorect"]:
            xy, m = np.zeros((J, 2)), 0
            for p in rect["annopoints"][0]["point"]:
                xy[p["id"][0]] = (p["x"][0], p["y"][0])
                m |= 1 << p["id"][0]
            gt_xy.append(xy), gt_has.append(m)
            gt_head.append([rect[c][0] for c in ("x1", "y1", "x2", "y2")])
        gt_off.append(len(gt_has))
        for region in fr.get("ignore_regions", []):
            vert_xy.extend((p["x"][0], p["y"][0]) for p in region["point"])
            vert_off.append(len(vert_xy))
        poly_off.append(len(vert_off) - 1)
    # the packed predictions: persons in frame order, -1 for the placeholder
    pr_off, pr_sample = [0], []
    for f in kept:
        s = np.nonzero(frame_id == f)[0]
        pr_sample.extend(s.tolist() if s.size else [-1])
        pr_off.append(len(pr_sample))

    n_gt_before = [len(fr["annorect"]) for fr in gt]
    gt, pr = E.removeIgnoredPoints(gt, pr)
    scoresAll, labelsAll, nGTall, _ = E.assignGTmulti(gt, pr, 0.5)
    apAll, preAll, recAll = E.compute_metrics(scoresAll, labelsAll, nGTall)
    table = E.getCum(apAll)

    # per frame and joint the reference's entries, laid out on the (person, joint) grid: the remaining rects carry their
    # original place in the frame as track_id (PoseTrackDataset.py:569)
    labels = np.full((len(pr_sample), J), -1, np.int8)
    scores = np.zeros((len(pr_sample), J))
    for i, fr in enumerate(pr):
        took = [0] * J
        for rect in fr["annorect"]:
            slot = pr_off[i] + rect["track_id"][0]
            for p in rect["annopoints"][0]["point"]:
                k = p["id"][0]
                labels[slot, k] = labelsAll[k][i][took[k]]
                scores[slot, k] = scoresAll[k][i][took[k]]
                assert scores[slot, k] == p["score"][0]
                took[k] += 1
        assert all(took[k] == len(labelsAll[k][i]) == len(scoresAll[k][i]) for k in range(J))

    arrays = dict(
        seed=np.int64(SEED), frames=np.int64(FRAMES), preds=preds, box_score=box, frame_id=frame_id,
        kept=np.asarray(kept, np.int64), pr_off=np.asarray(pr_off, np.int32), pr_sample=np.asarray(pr_sample, np.int32),
        gt_off=np.asarray(gt_off, np.int32), gt_xy=np.asarray(gt_xy, np.float64).reshape(-1, J, 2),
        gt_has=np.asarray(gt_has, np.int32), gt_head=np.asarray(gt_head, np.float64).reshape(-1, 4),
        poly_off=np.asarray(poly_off, np.int32), vert_off=np.asarray(vert_off, np.int32),
        vert_xy=np.asarray(vert_xy, np.float64).reshape(-1, 2),
        ann_off=np.asarray(ann_off, np.int32), ann_points=np.asarray(ann_pts, np.int32), ann_xy=np.asarray(ann_xy),
        ann_score=np.asarray(ann_score), ann_rect_score=np.asarray(ann_rect_score), ann_track=np.asarray(ann_track, np.int32),
        labels=labels, scores=scores, nGTall=nGTall.T.astype(np.int32), apAll=apAll[:, 0], preAll=preAll[:, 0],
        recAll=recAll[:, 0], table=np.asarray(table, np.float64))

    # ---- what the data must contain, and the conditions under which the reference alone is unambiguous ---------------
    a = arrays
    npr, ngp = np.diff(a["pr_off"]), np.diff(a["gt_off"])
    assert (a["pr_sample"] < 0).any(), "no frame without detections"
    assert any(b > 0 and len(fr["annorect"]) == 0 for b, fr in zip(n_gt_before, gt)), "no GT emptied by an ignore region"
    assert (a["gt_has"] == 0).any() and any((a["gt_has"][a["gt_off"][i]:a["gt_off"][i + 1]] == 0).any()
                                            and a["poly_off"][i] == a["poly_off"][i + 1] for i in range(len(kept))), \
        "no GT person with nGTp == 0"
    assert ((a["gt_has"] != 0) & (a["gt_has"] != 2 ** J - 1)).any(), "no GT person with a subset of joints"
    assert (npr > ngp).any() and npr.max() <= 8 and ngp.max() <= 6
    nv = np.diff(a["vert_off"])
    assert nv.size >= 4 and nv.min() >= 3, "ignore polygons are missing"
    lab_person = labels.max(1)
    assert (lab_person == 1).any() and (lab_person == 0).any() and (labels == -1).any()
    assert all(np.isfinite(v) for v in table) and (apAll > 0).all() and (apAll < 100).all()
    args = [a[k] for k in ("pr_off", "pr_sample")] + [preds[:, :, :2], preds[:, :, 2:], box] + \
        [a[k] for k in ("gt_off", "gt_xy", "gt_has", "gt_head", "poly_off", "vert_off", "vert_xy")]
    R.input_conditions(*args)                                        # (a) - (d) on the packed input
    for k in range(J):                                               # (b) on the reference's own entries
        s = np.concatenate([np.ravel(scoresAll[k][i]) for i in range(len(gt))])
        l = np.concatenate([np.ravel(labelsAll[k][i]) for i in range(len(gt))])
        order = np.argsort(s, kind="stable")
        s, l = s[order], l[order]
        assert not ((s[1:] == s[:-1]) & (l[1:] != l[:-1])).any(), "(b) equal scores with different labels"
    # cases read off the reference's own frames after removeIgnoredPoints, with its distance and head size
    competing = far = slot_kept = False
    for i, (g_fr, p_fr) in enumerate(zip(gt, pr)):
        G, P = g_fr["annorect"], p_fr["annorect"]
        tracks = [r["track_id"][0] for r in P]
        if P and len(tracks) < npr[i] and min(set(range(npr[i])) - set(tracks)) < max(tracks):
            slot_kept = True            # a predicted person lost every point to an ignore region, a later one remains
        if not (G and P):
            continue
        pck = np.zeros((len(P), len(G)))
        for gi, rg in enumerate(G):
            head = E.get_head_size(rg["x1"][0], rg["y1"][0], rg["x2"][0], rg["y2"][0])
            gpts = {q["id"][0]: (q["x"][0], q["y"][0]) for q in rg["annopoints"][0]["point"]}
            for pi, rp in enumerate(P):
                hit = sum(1 for q in rp["annopoints"][0]["point"] if q["id"][0] in gpts and
                          np.linalg.norm(np.subtract(gpts[q["id"][0]], [q["x"][0], q["y"][0]])) / head <= 0.5)
                pck[pi, gi] = hit / len(gpts) if gpts else hit
        best = pck.argmax(1)
        claims = np.bincount(best[pck.max(1) > 0], minlength=len(G))
        competing |= bool((claims >= 2).any())                       # two detections whose best GT is the same one
        far |= any(len(rp["annopoints"][0]["point"]) == J and pck[pi].max() == 0 for pi, rp in enumerate(P))
    assert competing, "no two detections competing for one GT"
    assert far, "no detection far from every GT"
    assert slot_kept, "no frame where an ignore region removed a predicted person in front of one that stays"
    path = os.path.join(HERE, "posetrack_ap.npz")
    save_deterministic(path, arrays)
    print(f"wrote {path} ({os.path.getsize(path) / 1e3:.1f} kB); table = {[round(v, 3) for v in table]}")
    assert os.path.getsize(path) < 300 * 1024


if __name__ == "__main__":
    main()
