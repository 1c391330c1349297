#!/usr/bin/env python
"""Generate tests/golden/crop.npz by IMPORTING the reference's crop helpers (build container only).

Run from the repo root:  ``python tests/golden/make_golden_crop.py``

The reference is imported with the stubs of make_golden.py (empty ``torchvision`` / ``cv2`` modules).  One more stub:
``cv2.getAffineTransform`` becomes a float64 solve of the three point pairs (the 6 x 6 system OpenCV builds, solved
by LAPACK) - OpenCV itself is absent here, so the vectors pin the float32 point construction around that call and the
solve as restated, not OpenCV's own LU.  Recorded:

- ``box2cs`` (utils/bbox.py) of wide, tall and exact-aspect boxes, enlarge 1 and 1.25;
- ``get_affine_transform`` (utils/transform.py) for rot in {0, 17.5, -40}, inv 0 and 1;
- ``exec_affine_transform`` of points through those matrices (numpy's dot: BLAS summation order);
- ``generate_heatmaps`` (utils/heatmap.py) for sigma 2 and 3 after the visibility cut of
  dataset/PoseTrackDataset.py:408-414 (restated below), joints at the edges, outside, at negative coordinates and
  invisible.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import import_reference, save     # noqa: E402


def _three_point_solve(src, dst):
    src = np.asarray(src, np.float64)
    dst = np.asarray(dst, np.float64)
    a = np.zeros((6, 6))
    for i in range(3):
        a[2 * i, 0:2] = src[i]
        a[2 * i, 2] = 1.0
        a[2 * i + 1, 3:5] = src[i]
        a[2 * i + 1, 5] = 1.0
    return np.linalg.solve(a, dst.reshape(6, 1)).reshape(2, 3)


def main():
    import_reference()
    sys.modules["cv2"].getAffineTransform = _three_point_solve
    import utils.bbox as BB
    import utils.heatmap as HM
    import utils.transform as TR

    out = {}
    image_size = np.array([288, 384])
    heatmap_size = np.array([72, 96])
    aspect = image_size[0] * 1.0 / image_size[1]

    # box -> center / scale: wide, tall, exact aspect, fractional, the center-x == -1 quirk
    boxes = np.array([[100.0, 50.0, 300.0, 120.0], [10.5, 20.25, 40.0, 300.0], [0.0, 0.0, 75.0, 100.0],
                      [-20.7, 613.3, 91.1, 77.9], [-51.0, 3.0, 100.0, 60.0], [1201.9, 33.3, 8.1, 13.7]])
    for k, enl in enumerate((1.0, 1.25)):
        cs = [BB.box2cs(b, aspect, enl) for b in boxes]
        out[f"box_center_{k}"] = np.stack([c for c, _ in cs])
        out[f"box_scale_{k}"] = np.stack([s for _, s in cs])
    out["boxes"] = boxes
    out["box_enlarge"] = np.array([1.0, 1.25])
    out["aspect"] = np.array([aspect])

    # crop matrices over those boxes (enlarge 1.25), three rotations, both directions
    centers, scales = out["box_center_1"], out["box_scale_1"]
    rots = np.array([0.0, 17.5, -40.0])
    trans = np.zeros((len(rots), 2, len(boxes), 2, 3))
    for i, r in enumerate(rots):
        for inv in (0, 1):
            for b in range(len(boxes)):
                trans[i, inv, b] = TR.get_affine_transform(centers[b], scales[b], r, image_size, inv=inv)
    out["rots"], out["trans"] = rots, trans

    # exec_affine_transform of seeded points through the forward matrices
    rng = np.random.RandomState(7)
    pts = rng.uniform(-100, 1400, size=(len(boxes), 17, 2))
    moved = np.zeros_like(pts)
    for b in range(len(boxes)):
        for j in range(17):
            moved[b, j] = TR.exec_affine_transform(pts[b, j], trans[1, 0, b])
    out["pts"], out["pts_moved"] = pts, moved

    # targets: crop-space joints (17) for each sigma
    J = 17
    joints = rng.uniform(0, 1, size=(4, J, 3)) * np.array([288.0, 384.0, 0.0])
    vis = np.ones((4, J, 3))
    edge = [(0.0, 0.0), (288.0, 384.0), (288.0, 0.0), (0.0, 384.0), (287.9, 383.9), (288.01, 10.0),
            (-0.01, 50.0), (-2.0, -3.0), (-30.0, 100.0), (310.0, 390.0), (143.99, 191.99), (1.99, 1.99)]
    for j, (x, y) in enumerate(edge):
        joints[0, j, :2] = (x, y)
    joints[1, :6, :2] = [(-5.0, 10.0), (10.0, -5.0), (-13.0, -13.0), (300.0, 40.0), (40.0, 400.0), (-7.9, 20.0)]
    vis[1, 3:6] = 0.0                                  # invisible (and far outside: never moved)
    vis[2, ::3] = 0.0
    joints[3, :, :2] = rng.uniform(-40, 420, size=(J, 2))
    for s_i, sigma in enumerate((2, 3)):
        tgts, wts, viss = [], [], []
        for b in range(4):
            jt, jv = joints[b].copy(), vis[b].copy()
            for j in range(J):                                     # the dataset's visibility cut
                x, y = jt[j, 0], jt[j, 1]
                if x < 0 or y < 0 or x > image_size[0] or y > image_size[1]:
                    jv[j] = 0
            t, w = HM.generate_heatmaps(jt, jv, sigma, image_size, heatmap_size, J, use_different_joints_weight=False)
            tgts.append(t)
            wts.append(w)
        out[f"target_s{sigma}"] = np.stack(tgts)
        out[f"target_weight_s{sigma}"] = np.stack(wts)
    out["joints"], out["joints_vis"] = joints, vis
    save("crop", **out)


if __name__ == "__main__":
    main()
