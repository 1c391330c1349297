#!/usr/bin/env python
"""A 64-frame pool from the detector's boxes to keypoints, two ways: the host recipe of INTEGRATION.md section 3b' (boxes to
the host, ``crop.box_to_center_scale`` / ``crop.window`` in numpy, ``OTPose.predict`` at the chunk's person count) and
``VideoPose`` (``ops.pose_plan`` on the device, the engine at one fixed batch).  The pool is walked in chunks of
``--chunk`` frames (plus a halo of two frames on each side for the windows); the person count changes from chunk to chunk.

Each pass over the pool is timed with HIP events on the launch stream and with the wall clock around a closing synchronise;
the two paths alternate, ``--passes`` times after one warm-up pass each.  Engine builds (a new ``model._engine``) are
counted per pass.  The detections are synthetic (seeded), so no detector weights are needed; both paths get the same ones and
their keypoints are compared.  Prints one line per figure and a JSON line."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from otpose_amd import OTPose, VideoPose, cfg2, tiny_cfg  # noqa: E402
from otpose_amd import crop as C  # noqa: E402
from otpose_amd import synthetic as S  # noqa: E402


def host_pass(model, pool, det, chunks, size):
    """The recipe of INTEGRATION.md section 3b' / 3b'-0 per chunk."""
    boxes, _, counts, _, _ = det
    frames = pool.shape[0]
    builds, last, out = 0, model._engine, []
    for lo, hi in chunks:
        cnt = counts[lo:hi].tolist()                                       # device -> host
        if sum(cnt) == 0:
            continue
        xywh = torch.cat([boxes[s, :cnt[s - lo]] for s in range(lo, hi)]).cpu().numpy()
        center, scale = C.box_to_center_scale(xywh, size[0] / size[1], enlarge=1.25)
        idx, margin = [], []
        for s in range(lo, hi):
            for _ in range(cnt[s - lo]):
                f, m = C.window(s, frames, posetrack18=True)
                idx.append(f)                                              # one video from frame 0: slot = frame number
                margin.append(m)
        out.append(model.predict(pool, idx, center, scale, torch.tensor(margin, dtype=torch.float32))[0])
        builds += model._engine is not last
        last = model._engine
    return torch.cat(out), builds


def device_pass(vp, pool, det, chunks):
    builds, last, out = 0, vp.model._engine, []
    for lo, hi in chunks:
        out.append(vp.run(pool, *det, detect=(lo, hi)).preds)
        builds += vp.model._engine is not last
        last = vp.model._engine
    return torch.cat(out), builds


def timed(fn):
    torch.cuda.synchronize()
    st = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record(st)
    res = fn()
    e1.record(st)
    e1.synchronize()
    torch.cuda.synchronize()
    return res, e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3     # ms, ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--chunk", type=int, default=8)
    ap.add_argument("--capacity", type=int, default=16)
    ap.add_argument("--max-per-frame", type=int, default=3)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--cfg", choices=("tiny", "cfg2"), default="tiny", help="tiny: width 16 at 128 x 192; cfg2: the full model")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("video_pose_bench needs the GPU")
    cfg = cfg2() if a.cfg == "cfg2" else tiny_cfg(16, (128, 192))
    size = tuple(cfg.MODEL.IMAGE_SIZE)
    rng = np.random.RandomState(0)
    n, k = a.frames, a.max_per_frame
    pool = torch.from_numpy(rng.randint(0, 256, (n, 720, 1280, 3)).astype(np.uint8)).cuda()
    counts = rng.randint(0, k + 1, n).astype(np.int32)
    boxes = np.stack([rng.uniform(0, 1100, (n, k)), rng.uniform(0, 500, (n, k)), rng.uniform(60, 300, (n, k)),
                      rng.uniform(100, 500, (n, k))], axis=2)
    scores = rng.uniform(0.5, 1.0, (n, k)).astype(np.float32)
    for s in range(n):
        boxes[s, counts[s]:], scores[s, counts[s]:] = 0, 0
    det = [torch.from_numpy(x).cuda() for x in (boxes, scores, counts, np.arange(n, dtype=np.int32), np.full(n, n, np.int32))]
    chunks = [(lo, min(lo + a.chunk, n)) for lo in range(0, n, a.chunk)]
    per_chunk = [int(counts[lo:hi].sum()) for lo, hi in chunks]

    def make():
        m = OTPose(cfg)
        S.fill_synthetic_(m)
        return m.cuda().eval()
    model = make()                               # one model per path (the same weights): neither evicts the other's engine
    vp = VideoPose(make(), a.capacity)
    res = {"frames": n, "chunk": a.chunk, "capacity": a.capacity, "cfg": a.cfg, "persons": int(counts.sum()),
           "persons_per_chunk": per_chunk, "passes": a.passes}
    rows = {"host": [], "device": []}
    with torch.no_grad():
        ref, _ = host_pass(model, pool, det, chunks, size)                    # warm-up passes (code objects, first graphs)
        got, _ = device_pass(vp, pool, det, chunks)
        res["max_abs_keypoint_difference_px"] = float((ref - got).abs().max())
        for _ in range(a.passes):
            for name, fn in (("host", lambda: host_pass(model, pool, det, chunks, size)),
                             ("device", lambda: device_pass(vp, pool, det, chunks))):
                (_, builds), ev_ms, wall_ms = timed(fn)
                rows[name].append((ev_ms, wall_ms, builds))
    for name, r in rows.items():
        res[name] = {"event_ms": [round(v[0], 2) for v in r], "wall_ms": [round(v[1], 2) for v in r],
                     "engine_builds": [v[2] for v in r]}
        print("%-6s pass: events %s ms, wall %s ms, engine builds %s" % (name, res[name]["event_ms"], res[name]["wall_ms"],
                                                                        res[name]["engine_builds"]))
    print("keypoints of the two paths differ by at most %.3g px" % res["max_abs_keypoint_difference_px"])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
