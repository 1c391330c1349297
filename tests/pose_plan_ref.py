"""numpy restatement of csrc/plan.hip (``ops.pose_plan``): the host recipe of INTEGRATION.md section 3b' - per person
``crop.box_to_center_scale``, ``crop.crop_matrix`` and ``crop.window`` - plus the compaction of the detector's (frame, box)
grid into dense rows.  No arithmetic of its own.

``M_MEASURED`` is the largest |closed form - crop.crop_matrix| over 10^5 random boxes (corner in 0..4096 px, sides in
8..4096 px, RandomState(0), aspect 288 / 384, enlarge 1.25, crops of 288 x 384), measured on the CPU with the closed form of
tests/test_pose_plan_host.py; the largest entry of those matrices is 7e4, so it is 5e-14 of it.  ``M_TOL`` = 16 x that is the
bound of every comparison of a closed-form matrix with the LAPACK solve: the margin covers another LAPACK build and the
order of the operations."""
from __future__ import annotations

import numpy as np

from otpose_amd import crop as C

M_MEASURED = 3.92e-9
M_TOL = 16 * M_MEASURED


def sequences(frame_number, num_frames):
    """Sequence id of every pool slot: a sequence is a run of slots with one num_frames and strictly increasing numbers."""
    fn, nf = np.asarray(frame_number), np.asarray(num_frames)
    seq = np.zeros(len(fn), np.int64)
    for t in range(1, len(fn)):
        seq[t] = seq[t - 1] + int(nf[t] != nf[t - 1] or fn[t] <= fn[t - 1])
    return seq


def pose_plan_ref(boxes, scores, counts, frame_number, num_frames, detect, min_score, aspect_ratio, enlarge, out_size,
                  posetrack18, max_persons):
    """Returns a dict with the arrays of ``ops.PosePlan`` (``total`` an int)."""
    boxes, scores = np.asarray(boxes, np.float64), np.asarray(scores)
    S, K = scores.shape
    fn, nf = [int(v) for v in frame_number], [int(v) for v in num_frames]
    seq = sequences(fn, nf)
    pool_slot = {(int(seq[t]), fn[t]): t for t in range(S)}                  # (sequence, frame number) -> pool slot
    lo, hi = detect
    P = int(max_persons)
    kept, pr_off = [], [0]
    for s in range(S):
        if lo <= s < hi:
            kept += [(s, k) for k in range(min(max(int(counts[s]), 0), K))
                     if not np.float64(scores[s, k]) < np.float64(min_score)]
        pr_off.append(min(len(kept), P))
    total = len(kept)
    rows = kept[:P]
    n = len(rows)
    out = {"center": np.zeros((P, 2), np.float32), "scale": np.zeros((P, 2), np.float32),
           "M": np.tile(np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]), (P, 1, 1)),
           "frame_idx": np.full((P, 5), -1, np.int32), "margin": np.zeros((P, 4), np.float32),
           "box_score": np.zeros(P, np.float64), "person_slot": np.full(P, -1, np.int32),
           "pr_off": np.array(pr_off, np.int32), "total": total}
    if n:
        b = np.stack([boxes[s, k] for s, k in rows])
        c, sc = C.box_to_center_scale(b, aspect_ratio, enlarge)
        out["center"][:n], out["scale"][:n] = c, sc
        out["M"][:n] = C.crop_matrix(c, sc, 0.0, out_size)
    for r, (s, k) in enumerate(rows):
        q = int(seq[s])
        frames, margin = C.window(fn[s], nf[s], distance=2, posetrack18=posetrack18,
                                  available=lambda f, q=q: (q, f) in pool_slot)
        out["frame_idx"][r] = [pool_slot.get((q, f), -1) for f in frames]
        out["margin"][r] = margin
        out["box_score"][r] = scores[s, k]
        out["person_slot"][r] = s
    return out
