"""numpy restatement of csrc/posenms.hip (the contract in include/otpose_hip.h) on the packed arrays: float64 element-wise
operations, every product, quotient and sum rounded on its own, the joint sums left to right.

``pose_nms_ref``: person scores, the OKS tile of every frame, hard / soft NMS; vectorised per frame.
``input_conditions``: the conditions under which a last-bit difference of ``exp`` cannot change a decision.
``hrnet_*``: a literal, loop-by-loop transcription of HRNet's lib/nms/nms.py (``oks_iou``, ``oks_nms``, ``rescore``,
``soft_oks_nms``) and of the rescoring loop of its COCO ``evaluate``, as the maintainers know them (HRNet's source was not at
hand: NOT VERIFIED against it).  Its two ``argsort()[::-1]`` are given ``kind="stable"``, which pins the order of ties the
contract states; HRNet's own is that of an unstable sort.
"""
from __future__ import annotations

import numpy as np

J = 17
MAX_PR = 64
COCO_SIGMAS = np.array([.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89]) / 10.0


def order_of(scores):
    """Descending; ties as a stable ascending sort followed by a reversal (the later person first), NaN before numbers."""
    return np.argsort(scores, kind="stable")[::-1]


def _persons(pr_sample, preds, maxvals, box_score, area):
    s = np.asarray(pr_sample, np.int64)
    real = s >= 0
    si = np.where(real, s, 0)
    preds = np.asarray(preds, np.float32).reshape(-1, J, 2)
    maxvals = np.asarray(maxvals, np.float32).reshape(-1, J)
    box, area = np.asarray(box_score, np.float64).reshape(-1), np.asarray(area, np.float64).reshape(-1)
    if preds.shape[0] == 0:
        preds, maxvals, box, area = np.zeros((1, J, 2), np.float32), np.zeros((1, J), np.float32), np.zeros(1), np.zeros(1)
    xy, v = preds[si].astype(np.float64), maxvals[si].astype(np.float64)
    box, area = box[si].copy(), area[si].copy()
    for a in (xy, v, box, area):                    # the placeholder person: a pose of zeros
        a[~real] = 0.0
    return xy, v, box, area, real


def person_scores(v, box, real, in_vis_thre):
    """box score x mean confidence of the joints above ``in_vis_thre`` (sum left to right), 0 for the placeholder."""
    kpt, n = np.zeros(v.shape[0]), np.zeros(v.shape[0], np.int64)
    for j in range(J):
        m = v[:, j] > in_vis_thre
        kpt = np.where(m, kpt + v[:, j], kpt)
        n += m
    kpt = np.where(n > 0, kpt / np.maximum(n, 1), kpt)
    with np.errstate(invalid="ignore"):
        return np.where(real, kpt * box, 0.0)


def oks_tile(xy, v, area, real, sigmas=COCO_SIGMAS, oks_in_vis_thre=None):
    """(n, n) float64: [g, d] = OKS of candidate d against kept person g; 0 for a pair with the placeholder."""
    var = (np.asarray(sigmas, np.float64) * 2) ** 2
    with np.errstate(all="ignore"):
        dx = xy[None, :, :, 0] - xy[:, None, :, 0]
        dy = xy[None, :, :, 1] - xy[:, None, :, 1]
        e = (dx ** 2 + dy ** 2) / var / ((area[:, None] + area[None, :]) / 2 + np.spacing(1))[..., None] / 2
        term = np.exp(-e)
        total, n = np.zeros(e.shape[:2]), np.zeros(e.shape[:2], np.int64)
        for j in range(J):
            sel = np.ones(e.shape[:2], bool) if oks_in_vis_thre is None else np.broadcast_to(
                v[None, :, j] > oks_in_vis_thre, e.shape[:2])
            total = np.where(sel, total + term[..., j], total)
            n += sel
        o = np.where(n > 0, total / np.maximum(n, 1), 0.0)
    return np.where(real[:, None] & real[None, :], o, 0.0)


def _decay(sc, o, thresh, soft_type):
    with np.errstate(all="ignore"):
        if soft_type == "gaussian":
            return sc * np.exp(-(o ** 2) / thresh)
        return np.where(o >= thresh, sc * (1 - o), sc)


def nms_frame(score, oks, real, oks_thresh, soft=False, soft_type="gaussian", max_dets=20, trace=None):
    """One frame -> (keep bool, out_score, rank).  ``trace`` collects what ``input_conditions`` looks at."""
    n = score.size
    keep, rank = np.zeros(n, bool), np.full(n, -1, np.int64)
    if not soft:
        order = order_of(score)
        rank[order] = np.arange(n)
        alive = np.ones(n, bool)
        for i, g in enumerate(order):
            if not alive[g]:
                continue
            keep[g] = True
            later = order[i + 1:]
            later = later[alive[later]]
            o = oks[g, later]
            if trace is not None:
                trace["oks"].append(o)
            with np.errstate(invalid="ignore"):
                alive[later] = o <= oks_thresh
        return keep | ~real, score.copy(), rank
    sc = score.copy()
    remaining = np.arange(n)                        # ascending person index, so the tie rule is the contract's
    for step in range(max_dets):
        if remaining.size == 0:
            break
        lead = remaining[order_of(sc[remaining])]
        if trace is not None and lead.size > 1:
            trace["lead"].append(sc[lead[:2]])
        g = lead[0]
        keep[g], rank[g] = True, step
        remaining = remaining[remaining != g]
        sc[remaining] = _decay(sc[remaining], oks[g, remaining], oks_thresh, soft_type)
    return keep | ~real, sc, rank


def pose_nms_ref(pr_off, pr_sample, preds, maxvals, box_score, area, *, oks_thresh, in_vis_thre=0.0, oks_in_vis_thre=None,
                 sigmas=COCO_SIGMAS, soft=False, soft_type="gaussian", max_dets=20, return_oks=False, trace=None):
    """-> (keep (NP,) bool, person_score (NP,) float64, rank (NP,) int32[, oks (NP, 64) float64]) as ``ops.pose_nms``."""
    pr_off = np.asarray(pr_off, np.int64)
    xy, v, box, ar, real = _persons(pr_sample, preds, maxvals, box_score, area)
    score = person_scores(v, box, real, in_vis_thre)
    npr = real.size
    keep, out, rank = np.zeros(npr, bool), np.zeros(npr), np.zeros(npr, np.int32)
    tiles = np.zeros((npr, MAX_PR))
    for a, b in zip(pr_off[:-1], pr_off[1:]):
        if b == a:
            continue
        o = oks_tile(xy[a:b], v[a:b], ar[a:b], real[a:b], sigmas, oks_in_vis_thre)
        tiles[a:b, :b - a] = o
        keep[a:b], out[a:b], rank[a:b] = nms_frame(score[a:b], o, real[a:b], oks_thresh, soft, soft_type, max_dets, trace)
    return (keep, out, rank, tiles) if return_oks else (keep, out, rank)


def input_conditions(pr_off, pr_sample, preds, maxvals, box_score, area, **settings):
    """Assert on the restatement's own values: (a) every OKS the greedy walk evaluates is at least 1e-9 away from
    ``oks_thresh`` (hard NMS; for the linear soft type the same holds for every OKS used in a decay), (b) at every soft step
    the two leading scores differ by at least 1e-9 relative or are bit-equal.  They constrain the generated input and exclude
    nothing from a comparison."""
    trace = {"oks": [], "lead": []}
    settings = dict(settings)
    thresh = settings["oks_thresh"]
    res = pose_nms_ref(pr_off, pr_sample, preds, maxvals, box_score, area, trace=trace, return_oks=True, **settings)
    if not settings.get("soft", False):
        o = np.concatenate(trace["oks"]) if trace["oks"] else np.zeros(0)
        assert not (np.abs(o - thresh) < 1e-9).any(), "(a) an OKS within 1e-9 of the threshold"
    else:
        if settings.get("soft_type", "gaussian") == "linear":
            o = res[3]
            assert not (np.abs(o - thresh) < 1e-9).any(), "(a) an OKS within 1e-9 of the threshold"
        for a, b in trace["lead"]:
            same = a.tobytes() == b.tobytes() or (np.isnan(a) and np.isnan(b))
            with np.errstate(invalid="ignore"):
                apart = np.isnan(a) != np.isnan(b) or abs(a - b) >= 1e-9 * max(abs(a), abs(b))
            assert same or apart, f"(b) leading soft scores {a!r} and {b!r}"
    return res


# ---- HRNet, transcribed ------------------------------------------------------------------------------------------------

def hrnet_oks_iou(g, d, a_g, a_d, sigmas=None, in_vis_thre=None):
    if not isinstance(sigmas, np.ndarray):
        sigmas = np.array([.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89]) / 10.0
    vars = (sigmas * 2) ** 2
    xg = g[0::3]
    yg = g[1::3]
    vg = g[2::3]
    ious = np.zeros((d.shape[0]))
    for n_d in range(0, d.shape[0]):
        xd = d[n_d, 0::3]
        yd = d[n_d, 1::3]
        vd = d[n_d, 2::3]
        dx = xd - xg
        dy = yd - yg
        e = (dx ** 2 + dy ** 2) / vars / ((a_g + a_d[n_d]) / 2 + np.spacing(1)) / 2
        if in_vis_thre is not None:
            ind = list(vg > in_vis_thre) and list(vd > in_vis_thre)
            e = e[ind]
        ious[n_d] = np.sum(np.exp(-e)) / e.shape[0] if e.shape[0] != 0 else 0.0
    return ious


def hrnet_oks_nms(kpts_db, thresh, sigmas=None, in_vis_thre=None):
    if len(kpts_db) == 0:
        return []
    scores = np.array([kpts_db[i]['score'] for i in range(len(kpts_db))])
    kpts = np.array([kpts_db[i]['keypoints'].flatten() for i in range(len(kpts_db))])
    areas = np.array([kpts_db[i]['area'] for i in range(len(kpts_db))])
    order = scores.argsort(kind="stable")[::-1]
    keep = []
    while order.size > 0:
        i = order[0]
        keep.append(i)
        oks_ovr = hrnet_oks_iou(kpts[i], kpts[order[1:]], areas[i], areas[order[1:]], sigmas, in_vis_thre)
        inds = np.where(oks_ovr <= thresh)[0]
        order = order[inds + 1]
    return keep


def hrnet_rescore(overlap, scores, thresh, type='gaussian'):
    assert overlap.shape[0] == scores.shape[0]
    if type == 'linear':
        inds = np.where(overlap >= thresh)[0]
        scores[inds] = scores[inds] * (1 - overlap[inds])
    else:
        scores = scores * np.exp(- overlap ** 2 / thresh)
    return scores


def hrnet_soft_oks_nms(kpts_db, thresh, sigmas=None, in_vis_thre=None, type='gaussian', max_dets=20):
    """Returns (keep, the score each kept person had when it was taken).  HRNet fixes ``max_dets = 20`` and the gaussian
    type inside the function and returns ``keep`` alone; its re-sort orders ties by position in the CURRENT order, which
    the contract replaces by the person index - the two agree where no two remaining scores are equal."""
    if len(kpts_db) == 0:
        return [], []
    scores = np.array([kpts_db[i]['score'] for i in range(len(kpts_db))])
    kpts = np.array([kpts_db[i]['keypoints'].flatten() for i in range(len(kpts_db))])
    areas = np.array([kpts_db[i]['area'] for i in range(len(kpts_db))])
    order = scores.argsort(kind="stable")[::-1]
    scores = scores[order]
    keep = np.zeros(max_dets, dtype=np.intp)
    taken = np.zeros(max_dets)
    keep_cnt = 0
    while order.size > 0 and keep_cnt < max_dets:
        i = order[0]
        taken[keep_cnt] = scores[0]
        oks_ovr = hrnet_oks_iou(kpts[i], kpts[order[1:]], areas[i], areas[order[1:]], sigmas, in_vis_thre)
        order = order[1:]
        scores = hrnet_rescore(oks_ovr, scores[1:], thresh, type)
        tmp = scores.argsort(kind="stable")[::-1]
        order = order[tmp]
        scores = scores[tmp]
        keep[keep_cnt] = i
        keep_cnt += 1
    return keep[:keep_cnt], taken[:keep_cnt]


def hrnet_rescore_persons(img_kpts, in_vis_thre, num_joints=J):
    """The rescoring loop of HRNet's COCO ``evaluate``: in place, ``score`` = box score x mean visible-joint confidence."""
    for n_p in img_kpts:
        box_score = n_p['score']
        kpt_score = 0
        valid_num = 0
        for n_jt in range(0, num_joints):
            t_s = n_p['keypoints'][n_jt][2]
            if t_s > in_vis_thre:
                kpt_score = kpt_score + t_s
                valid_num = valid_num + 1
        if valid_num != 0:
            kpt_score = kpt_score / valid_num
        n_p['score'] = kpt_score * box_score
