"""numpy restatement of csrc/poseval.hip on the packed arrays (float64 element-wise operations, every product and sum
rounded on its own), for inputs larger than tests/golden/posetrack_ap.npz can hold.

``pose_assign_ref``: removeIgnoredPoints + assignGTmulti of reference utils/evaluate.py:22-67, 467-682.
``ap_curve_ref``: compute_metrics / compute_rpc / vocap (:686-751).
``input_conditions``: the conditions under which the reference alone is unambiguous (asserted on generated inputs).
"""
from __future__ import annotations

import numpy as np

J = 15
COCO_OF_OFFICIAL = np.array([16, 14, 12, 11, 13, 15, 10, 8, 6, 5, 7, 9, 1, 0, 2])


def in_polygon(px, py, verts):
    """Even-odd crossing test of points (n,) against one polygon (v,2), the arithmetic of csrc/poseval.hip in_any_polygon."""
    xi, yi = verts[:, 0][None, :], verts[:, 1][None, :]
    xj, yj = np.roll(verts[:, 0], 1)[None, :], np.roll(verts[:, 1], 1)[None, :]
    px, py = px[:, None], py[:, None]
    straddle = (yi > py) != (yj > py)
    with np.errstate(divide="ignore", invalid="ignore"):
        xc = (xj - xi) * (py - yi) / (yj - yi) + xi
    return (np.count_nonzero(straddle & (px < xc), axis=1) & 1).astype(bool)


def edge_distance(px, py, verts):
    """Smallest distance of points (n,) to the edges of one polygon (v,2)."""
    a = verts[None, :, :]
    b = np.roll(verts, 1, axis=0)[None, :, :]
    p = np.stack([px, py], -1)[:, None, :]
    ab = b - a
    den = (ab * ab).sum(-1)
    t = np.clip(((p - a) * ab).sum(-1) / np.where(den > 0, den, 1.0), 0.0, 1.0)
    d = p - (a + t[..., None] * ab)
    return np.sqrt((d * d).sum(-1)).min(1)


def _persons(pr_sample, preds, maxvals, box_score):
    s = np.asarray(pr_sample, np.int64)
    real = s >= 0
    si = np.where(real, s, 0)
    preds = np.asarray(preds, np.float32).reshape(-1, 17, 2)
    maxvals = np.asarray(maxvals, np.float32).reshape(-1, 17)
    box = np.asarray(box_score, np.float64).reshape(-1)
    if preds.shape[0] == 0:
        preds, maxvals, box = np.zeros((1, 17, 2), np.float32), np.zeros((1, 17), np.float32), np.zeros(1)
    xy = preds[si][:, COCO_OF_OFFICIAL, :].astype(np.float64)
    sc = maxvals[si][:, COCO_OF_OFFICIAL].astype(np.float64) * box[si][:, None]
    has = np.ones((s.size, J), bool)
    xy[~real] = 0.0                                 # the placeholder person: joint 0 at (0, 0), score -100
    sc[~real] = -100.0
    has[~real] = False
    has[~real, 0] = True
    return xy, sc, has


def _frame_of(off):
    return np.repeat(np.arange(off.size - 1), np.diff(off))


def removed_by_ignore(pr_off, pxy, phas, gt_off, gxy, ghas, poly_off, vert_off, vert_xy, margin=None):
    """Clears ``phas`` / ``ghas`` in place for points strictly inside an ignore polygon of their frame; with ``margin``
    returns the smallest point-to-edge distance met instead of nothing."""
    closest = np.inf
    for f in np.nonzero(np.diff(poly_off) > 0)[0]:
        for has, xy, off in ((phas, pxy, pr_off), (ghas, gxy, gt_off)):
            a, b = off[f], off[f + 1]
            if b == a:
                continue
            x, y = xy[a:b, :, 0].reshape(-1), xy[a:b, :, 1].reshape(-1)
            inside = np.zeros(x.size, bool)
            for q in range(poly_off[f], poly_off[f + 1]):
                v = vert_xy[vert_off[q]:vert_off[q + 1]]
                inside |= in_polygon(x, y, v)
                if margin is not None:
                    h = has[a:b].reshape(-1)
                    if h.any():
                        closest = min(closest, edge_distance(x[h], y[h], v).min())
            if margin is None:
                has[a:b] &= ~inside.reshape(-1, J)
    return closest


def pose_assign_ref(pr_off, pr_sample, preds, maxvals, box_score, gt_off, gt_xy, gt_has, gt_head, poly_off, vert_off,
                    vert_xy, dist_thresh=0.5, return_dist=False):
    """-> (labels (NP,15) int8, scores (NP,15) float64, ngt (F,15) int32); with ``return_dist`` also every finite
    normalised distance that was compared with the threshold."""
    pr_off, gt_off, poly_off = (np.asarray(a, np.int64) for a in (pr_off, gt_off, poly_off))
    vert_off = np.asarray(vert_off, np.int64)
    vert_xy = np.asarray(vert_xy, np.float64).reshape(-1, 2)
    F = pr_off.size - 1
    pxy, score, phas = _persons(pr_sample, preds, maxvals, box_score)
    gxy = np.asarray(gt_xy, np.float64).reshape(-1, J, 2)
    ghas = ((np.asarray(gt_has, np.int64).reshape(-1)[:, None] >> np.arange(J)) & 1).astype(bool)
    hd = np.asarray(gt_head, np.float64).reshape(-1, 4)
    dx, dy = hd[:, 2] - hd[:, 0], hd[:, 3] - hd[:, 1]
    head = 0.6 * np.sqrt(dx * dx + dy * dy)
    removed_by_ignore(pr_off, pxy, phas, gt_off, gxy, ghas, poly_off, vert_off, vert_xy)
    filtered = np.diff(poly_off) > 0
    pf, gf = _frame_of(pr_off), _frame_of(gt_off)
    palive = ~filtered[pf] | phas.any(1)
    galive = ~filtered[gf] | ghas.any(1)
    ngt = np.zeros((F, J), np.int64)
    np.add.at(ngt, gf, ghas.astype(np.int64))
    labels = np.where(phas, 0, -1).astype(np.int8)
    scores = np.where(phas, score, 0.0)
    dists = []

    npr, ngp = np.diff(pr_off), np.diff(gt_off)
    todo = np.nonzero((npr > 0) & (ngp > 0))[0]
    pad = lambda n: 1 << int(n - 1).bit_length() if n > 1 else 1
    key = np.array([pad(npr[f]) * 1024 + pad(ngp[f]) for f in todo], np.int64)
    for k in np.unique(key):
        P, G = int(k) // 1024, int(k) % 1024
        group = todo[key == k]
        step = max(1, (1 << 21) // (P * G * J))
        for c in range(0, group.size, step):
            fr = group[c:c + step]
            B = fr.size
            pi = pr_off[fr][:, None] + np.arange(P)[None, :]
            gi = gt_off[fr][:, None] + np.arange(G)[None, :]
            pv, gv = np.arange(P)[None, :] < npr[fr][:, None], np.arange(G)[None, :] < ngp[fr][:, None]
            pi, gi = np.where(pv, pi, 0), np.where(gv, gi, 0)
            pa, ga = pv & palive[pi], gv & galive[gi]
            ph, gh = phas[pi] & pa[..., None], ghas[gi] & ga[..., None]
            ddx = gxy[gi][:, None, :, :, 0] - pxy[pi][:, :, None, :, 0]
            ddy = gxy[gi][:, None, :, :, 1] - pxy[pi][:, :, None, :, 1]
            both = ph[:, :, None, :] & gh[:, None, :, :]
            with np.errstate(divide="ignore", invalid="ignore"):
                d = np.sqrt(ddx * ddx + ddy * ddy) / head[gi][:, None, :, None]
                match = both & (d <= dist_thresh)
            if return_dist:
                dists.append(d[both & np.isfinite(d)])
            cnt = match.sum(3).astype(np.float64)
            n = gh.sum(2)[:, None, :].astype(np.float64)
            pck = np.where(n > 0, cnt / np.where(n > 0, n, 1.0), cnt)
            pck = np.where(ga[:, None, :], pck, -1.0)                 # removed GT persons are not in the lists
            best = pck.argmax(2)
            keep = (np.arange(G)[None, None, :] == best[..., None]) & pa[..., None] & ga[:, None, :]
            kept = np.where(keep, pck, 0.0)
            to_gt = kept.argmax(1)                                       # (B, G): the predicted person of each GT
            val = kept.max(1)
            assign = np.full((B, P), -1, np.int64)
            b, g = np.nonzero((val > 0) & ga)
            assign[b, to_gt[b, g]] = g
            got = match[np.arange(B)[:, None], np.arange(P)[None, :], np.maximum(assign, 0)]      # (B, P, J)
            lab = np.where(assign[..., None] >= 0, got, False) & ga.any(1)[:, None, None]
            lab = np.where(ph, lab.astype(np.int8), -1).astype(np.int8)
            labels[pi[pv]] = lab[pv]
    out = labels, scores, ngt.astype(np.int32)
    return out + (np.concatenate(dists) if dists else np.zeros(0),) if return_dist else out


def sort_entries_ref(labels, scores):
    """Per joint the entries (label >= 0) by descending score, ties as a stable ascending sort followed by a reversal."""
    out = []
    for j in range(J):
        m = labels[:, j] >= 0
        s, l = scores[m, j], labels[m, j]
        idx = np.argsort(s, kind="stable")[::-1]
        out.append((l[idx], s[idx]))
    return out


def ap_curve_ref(labels, scores, ngt):
    """-> (ap, precision, recall), each (16,) float64: 15 joints x 100 and the mean over the joints that are not NaN."""
    res = np.zeros((3, J + 1))
    total = np.asarray(ngt, np.int64).sum(0).astype(np.float64)
    for j, (l, _) in enumerate(sort_entries_ref(labels, scores)):
        if l.size == 0:
            continue
        npos = np.cumsum(l == 1).astype(np.float64)
        prec = npos / np.arange(1, l.size + 1, dtype=np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            rec = npos / total[j]
        mpre = np.concatenate([[0.0], prec, [0.0]])
        mpre = np.maximum.accumulate(mpre[::-1])[::-1]
        mrec = np.concatenate([[0.0], rec, [1.0]])
        i = np.nonzero(~np.equal(mrec[1:], mrec[:-1]))[0] + 1
        with np.errstate(invalid="ignore"):
            res[0, j] = np.sum((mrec[i] - mrec[i - 1]) * mpre[i]) * 100
        res[1, j] = prec[-1] * 100
        res[2, j] = rec[-1] * 100
    for r in res:
        v = r[:J]
        r[J] = v[~np.isnan(v)].mean()
    return res[0], res[1], res[2]


def input_conditions(pr_off, pr_sample, preds, maxvals, box_score, gt_off, gt_xy, gt_has, gt_head, poly_off, vert_off,
                     vert_xy, dist_thresh=0.5):
    """Assert the conditions under which the reference alone is unambiguous; they constrain the generated input and exclude
    nothing from a comparison.  (a) no |dist - thresh| < 1e-9 (np.linalg.norm may or may not contract to an FMA), (b) within
    a joint no two entries of equal score and different label (the reference's argsort is unstable), (c) no point within
    1e-6 px of an ignore polygon's edge (shapely and the crossing test could differ there), (d) every head box has a
    non-zero size.  Returns the largest number of entries of one joint."""
    pr_off, gt_off, poly_off, vert_off = (np.asarray(a, np.int64) for a in (pr_off, gt_off, poly_off, vert_off))
    labels, scores, _, dist = pose_assign_ref(pr_off, pr_sample, preds, maxvals, box_score, gt_off, gt_xy, gt_has, gt_head,
                                              poly_off, vert_off, vert_xy, dist_thresh, return_dist=True)
    assert not (np.abs(dist - dist_thresh) < 1e-9).any(), "(a) a distance within 1e-9 of the threshold"
    most = 0
    for l, s in sort_entries_ref(labels, scores):
        most = max(most, l.size)
        same = s[1:] == s[:-1]
        assert not (same & (l[1:] != l[:-1])).any(), "(b) equal scores with different labels"
    pxy, _, phas = _persons(pr_sample, preds, maxvals, box_score)
    gxy = np.asarray(gt_xy, np.float64).reshape(-1, J, 2)
    ghas = ((np.asarray(gt_has, np.int64).reshape(-1)[:, None] >> np.arange(J)) & 1).astype(bool)
    closest = removed_by_ignore(pr_off, pxy, phas, gt_off, gxy, ghas, poly_off, vert_off,
                                np.asarray(vert_xy, np.float64).reshape(-1, 2), margin=1e-6)
    assert closest >= 1e-6, f"(c) a point {closest} px from a polygon edge"
    hd = np.asarray(gt_head, np.float64).reshape(-1, 4)
    assert ((hd[:, 2] != hd[:, 0]) | (hd[:, 3] != hd[:, 1])).all(), "(d) a head box of zero size"
    return most
