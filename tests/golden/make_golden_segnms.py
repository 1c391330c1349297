#!/usr/bin/env python
"""Generate tests/golden/segnms.npz by RUNNING the reference's temporal segment NMS (build container only).

Run from the repo root:  ``python tests/golden/make_golden_segnms.py``

The reference's ``thirdparty/utils/csrc/nms_cpu.cpp`` is built with ``torch.utils.cpp_extension.load`` into a directory
under the system's temporary folder (nothing compiled from it enters the repository), registered as ``nms_1d_cpu``, and
``thirdparty/utils/nms.py`` is loaded against it from its file.  Every recorded output is the reference's; on every case the
restatement tests/segnms_ref.py is asserted to reproduce the extension BIT FOR BIT (indices, segments, decayed scores).  If the
extension cannot be built the restatement alone is the yardstick, and ``yardstick`` in the file says which it was.

Kernel-level batch ``a``: one flat batch of groups with 0, 1, 2, 63, 64, 65, 200 and 1025 segments, a group of identical
segments, a group of disjoint ones and a group with zero-length segments.  Hard NMS at min_score 0 and 0.3, soft NMS for
(method, min_score) in SOFT_RUNS, voting of the hard-NMS survivors.  Method 0 with min_score 0 leaves suppressed segments
alive with the score 0 (``0 < 0`` is false) - equal scores, whose order the reference leaves to its array permutation - so
that pair runs on batch ``b`` (empty, single, disjoint), where nothing is suppressed.  ``max_num`` cuts (0, 1, larger than
the kept count) are asserted here to be prefixes of the uncut result, so the uncut result is what is stored.

Python-level cases: ``batched_nms`` multiclass with 1, 3 and 20 class ids (some never used), class-agnostic with and without
voting, each soft and hard at two ``min_score``; the three multiclass inputs together are the three-video batch.  The
reference's ``batched_nms`` hands ``NMSop.apply`` its scores and class ids in each other's place (see ``main``); the recorded
hard-NMS results are its code with that call put right.

The margins that make every discrete decision well defined are ASSERTED: at every selection the two highest live scores
differ by >= 1e-4 relative; every tested ovr (and voting iou) is >= 1e-3 from its threshold; every tested score is >= 1e-4
relative from min_score; input scores are pairwise distinct; neighbours of the final sort differ by >= 1e-4 relative; no
emitted score is below 1e-30.  The data of a group (or case) comes from one seed; a seed that fails a margin is skipped for
the next one (``seeds`` in the file records the ones used) - the margins never move.
"""
from __future__ import annotations

import importlib.util
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import REF, save                             # noqa: E402
from tests import segnms_ref as R                             # noqa: E402

F = np.float32
IOU, SIGMA, VOTE = 0.5, 0.5, 0.75
HARD_RUNS = (0.0, 0.3)                                        # min_score
SOFT_RUNS = ((0, 0.3), (1, 0.0), (1, 0.3), (2, 0.0), (2, 0.3))   # (method, min_score)
GROUPS_A = (("n0", 0), ("n1", 1), ("n2", 2), ("n63", 63), ("n64", 64), ("n65", 65), ("n200", 200), ("n1025", 1025),
            ("identical", 4), ("disjoint", 16), ("zero", 7))
GROUPS_B = (("n0", 0), ("n1", 1), ("disjoint", 16))
PY_CASES = (("mc1", 40, (7,)), ("mc3", 60, (0, 2, 5)), ("mc20", 150, (0, 1, 3, 4, 6, 7, 8, 10, 11, 13, 14, 16, 17, 19)),
            ("agn", 80, (0, 1, 2)))
PY_RUNS = ((True, 0.001), (True, 0.3), (False, 0.0), (False, 0.3))   # (use_soft_nms, min_score)
MAX_SEG = 100
LIMITS = {"top2": 1e-4, "ovr": 1e-3, "min_score": 1e-4, "distinct": 1e-7, "vote": 1e-3, "final": 1e-4}


def ladder(rs, n, lo, hi):
    return (np.linspace(lo, hi, n) + rs.uniform(-0.2, 0.2, n) * (hi - lo) / max(n, 1))[rs.permutation(n)].astype(F)


def make_group(kind, n, seed):
    """(segs (n, 2), scores (n)) float32 of one group."""
    rs = np.random.RandomState(seed)
    if kind == "identical":
        return np.tile(np.array([[10.0, 20.0]], F), (n, 1)), ladder(rs, n, 0.4, 0.9)
    if kind == "disjoint":
        x1 = (np.arange(n) * 10 + rs.uniform(0, 2, n)).astype(F)
        return np.stack([x1, x1 + rs.uniform(1, 6, n).astype(F)], 1)[rs.permutation(n)], ladder(rs, n, 0.05, 0.99)
    if kind == "zero":                                       # three zero-length segments: alone, inside a long one, twice at one place
        segs = np.array([[5, 5], [12, 12], [12, 12], [10, 20], [11, 19], [30, 42], [33, 44]], F)
        return segs, ladder(rs, n, 0.35, 0.95)
    if n <= 65:                                              # one crowded timeline
        c, l = rs.uniform(0, 3 * n + 10, n), rs.uniform(2, 12, n)
        return np.stack([c - l / 2, c + l / 2], 1).astype(F), ladder(rs, n, 0.05, 0.99)
    # large groups: disjoint singles in the upper score band, ten clusters of four in the lower one (a decayed score stays
    # below the singles, so the 1e-4 selection margin is a matter of the 40 clustered segments, not of n^2 pairs)
    k = n - 40
    x1 = np.arange(k) * 20 + rs.uniform(0, 5, k)
    singles = np.stack([x1, x1 + rs.uniform(2, 10, k)], 1)
    cc = 20 * k + 100 + np.repeat(np.arange(10) * 100, 4) + rs.uniform(-6, 6, 40)
    cl = rs.uniform(10, 30, 40)
    segs = np.concatenate([singles, np.stack([cc - cl / 2, cc + cl / 2], 1)]).astype(F)
    scores = np.concatenate([ladder(rs, k, 0.6, 0.99), ladder(rs, 40, 0.05, 0.55)])
    p = rs.permutation(n)
    return segs[p], scores[p]


def group_runs(segs, scores, soft_runs, margins):
    """Every kernel-level result of one group by the restatement."""
    out = {}
    for ms in HARD_RUNS:                                     # the segment's own index rides along as its "class"
        out["hard", ms] = R.NMSop_apply(segs, np.arange(len(scores)), scores, IOU, ms, 0, margins)
    for method, ms in soft_runs:
        dets, inds = R.softnms_1d(segs, scores, IOU, SIGMA, ms, method, margins)
        out["soft", method, ms] = dets[:len(inds)], inds
        assert len(inds) == 0 or dets[:len(inds), 2].min() >= (1e-30 if ms > 0 or method else 0.0)
    kept = R.nms_1d(segs, scores, IOU)
    out["vote"] = R.seg_voting(segs[kept], segs, scores, VOTE, margins=margins), kept
    return out


def margins_ok(m):
    return all(m.get(k, np.inf) >= v for k, v in LIMITS.items())


def search(build, first_seed, what):
    for seed in range(first_seed, first_seed + 2000):
        m = {}
        res = build(seed, m)
        if margins_ok(m):
            print(f"{what}: seed {seed}, margins", {k: float(f"{v:.3g}") for k, v in m.items()})
            return seed, res, m
    raise AssertionError(f"{what}: no seed in 2000 keeps the margins")


def load_reference():
    """(extension or None, the reference's nms.py module or None)."""
    try:
        from torch.utils.cpp_extension import load
        build_dir = os.path.join(tempfile.gettempdir(), "otpose_segnms_ext")
        os.makedirs(build_dir, exist_ok=True)
        ext = load(name="nms_1d_cpu", sources=[os.path.join(REF, "thirdparty", "utils", "csrc", "nms_cpu.cpp")],
                   build_directory=build_dir, verbose=False)
    except Exception as e:                                     # no compiler, no ninja: the restatement is the yardstick
        print("extension not built:", e)
        return None, None
    sys.modules["nms_1d_cpu"] = ext
    spec = importlib.util.spec_from_file_location("reference_nms", os.path.join(REF, "thirdparty", "utils", "nms.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return ext, mod


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def check_group_against_extension(ext, mod, segs, scores, soft_runs, runs):
    ts, tp = torch.from_numpy(segs), torch.from_numpy(scores)
    tc = torch.zeros(len(scores), dtype=torch.int64)
    assert same(ext.nms(ts, tp, IOU).numpy(), R.nms_1d(segs, scores, IOU))
    for ms in HARD_RUNS:
        mine = runs["hard", ms]
        for max_num in (0, 1, 5000):
            ref = mod.NMSop.apply(ts, tc, tp, IOU, ms, max_num)
            cut = len(mine[1]) if max_num == 0 else min(max_num, len(mine[1]))
            assert same(ref[0].numpy(), mine[0][:cut]) and same(ref[1].numpy(), mine[1][:cut])
    for method, ms in soft_runs:
        dets = torch.zeros((len(scores), 3))
        inds = ext.softnms(ts, tp, dets, IOU, SIGMA, ms, method).numpy()
        mine_d, mine_i = runs["soft", method, ms]
        assert same(inds, mine_i), (method, ms)
        assert same(dets[:len(inds)].numpy(), mine_d), (method, ms)
        for max_num in (1, 5000):                               # SoftNMSop's cut is a prefix
            ref = mod.SoftNMSop.apply(ts, tp, tc, IOU, SIGMA, ms, method, max_num)
            cut = min(max_num, len(inds))
            assert same(ref[0].numpy(), mine_d[:cut, :2]) and same(ref[1].numpy(), mine_d[:cut, 2])
    voted, kept = runs["vote"]
    if len(scores):
        ref = mod.seg_voting(ts[kept], ts, tp, VOTE).numpy()
        ok = np.isnan(ref) == np.isnan(voted)
        assert ok.all() and np.allclose(ref, voted, rtol=1e-5, atol=0, equal_nan=True)
        return ref
    return voted


def build_batch(name, groups, soft_runs, ext, mod, out, seeds):
    segs_l, scores_l, results = [], [], []
    for g, (kind, n) in enumerate(groups):
        k = kind if kind in ("identical", "disjoint", "zero") else "n"

        def build(seed, m, k=k, n=n):
            segs, scores = make_group(k, n, seed)
            return segs, scores, group_runs(segs, scores, soft_runs, m)

        seed, (segs, scores, runs), _ = search(build, 100 * (g + 1), f"{name}/{kind}")
        seeds[f"{name}/{kind}"] = seed
        if ext is not None:
            runs["vote"] = check_group_against_extension(ext, mod, segs, scores, soft_runs, runs), runs["vote"][1]
        segs_l.append(segs.reshape(-1, 2))
        scores_l.append(scores)
        results.append(runs)
    sizes = [len(s) for s in scores_l]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    N = int(off[-1])
    out[f"{name}_segs"], out[f"{name}_scores"], out[f"{name}_offsets"] = np.concatenate(segs_l), np.concatenate(scores_l), off
    for ms in HARD_RUNS:
        keep, counts = np.full(N, -1, np.int32), np.zeros(len(groups), np.int32)
        for g, runs in enumerate(results):
            idx = runs["hard", ms][2]
            counts[g] = len(idx)
            keep[off[g]:off[g] + len(idx)] = idx
        out[f"{name}_hard_ms{ms}_counts"], out[f"{name}_hard_ms{ms}_keep"] = counts, keep
    for method, ms in soft_runs:
        dets, inds, counts = np.zeros((N, 3), F), np.full(N, -1, np.int32), np.zeros(len(groups), np.int32)
        for g, runs in enumerate(results):
            d, i = runs["soft", method, ms]
            counts[g] = len(i)
            dets[off[g]:off[g] + len(i)], inds[off[g]:off[g] + len(i)] = d, i
        tag = f"{name}_soft_m{method}_ms{ms}"
        out[tag + "_counts"], out[tag + "_dets"], out[tag + "_inds"] = counts, dets, inds
    out[f"{name}_vote"] = np.concatenate([r["vote"][0].reshape(-1, 2) for r in results]).astype(F)


def make_case(n, ids, seed):
    rs = np.random.RandomState(seed)
    c, l = rs.uniform(0, 100, n), rs.uniform(5, 30, n)
    segs = np.stack([c - l / 2, c + l / 2], 1).astype(F)
    scores = rs.uniform(0.05, 0.99, n).astype(F)
    cls = np.array(ids, np.int64)[rs.randint(0, len(ids), n)]
    return segs, scores, cls


def case_runs(name, segs, scores, cls, fn, m=None):
    res = {}
    for soft, ms in PY_RUNS:
        variants = [(True, 0.0, MAX_SEG)] if name != "agn" else [(False, VOTE, MAX_SEG), (False, 0.0, 5)]
        for multiclass, vote, max_seg in variants:
            key = f"py_{name}_soft{int(soft)}_ms{ms}_vote{vote}_max{max_seg}"
            kw = dict(use_soft_nms=soft, multiclass=multiclass, sigma=SIGMA, voting_thresh=vote)
            res[key] = fn(segs, scores, cls, IOU, ms, max_seg, **kw) if m is None else fn(segs, scores, cls, IOU, ms, max_seg,
                                                                                         margins=m, **kw)
    return res


def main():
    ext, mod = load_reference()
    out, seeds = {}, {}
    out["yardstick"] = np.array("extension" if ext is not None else "restatement")
    build_batch("a", GROUPS_A, SOFT_RUNS, ext, mod, out, seeds)
    build_batch("b", GROUPS_B, ((0, 0.0),), ext, mod, out, seeds)

    if mod is not None:
        # nms.py:142-149 and 170-173 call NMSop.apply(segs, scores, cls_idxs, ...) while its forward reads (segs, cls_idxs,
        # scores, ...): the reference's hard path of batched_nms suppresses by CLASS ID and returns the two swapped.  That is
        # not recorded.  The reference's own batched_nms runs here with the call's arguments put where forward reads them.
        ref_nms_op = mod.NMSop

        class ArgumentOrder:
            @staticmethod
            def apply(segs, scores, cls_idxs, iou_threshold, min_score, max_num):
                return ref_nms_op.apply(segs, cls_idxs, scores, iou_threshold, min_score, max_num)

        mod.NMSop = ArgumentOrder

    for i, (name, n, ids) in enumerate(PY_CASES):
        def build(seed, m, name=name, n=n, ids=ids):
            segs, scores, cls = make_case(n, ids, seed)
            return segs, scores, cls, case_runs(name, segs, scores, cls, R.batched_nms, m)

        seed, (segs, scores, cls, mine), _ = search(build, 5000 + 1000 * i, f"py/{name}")
        seeds[f"py/{name}"] = seed
        out[f"py_{name}_in_segs"], out[f"py_{name}_in_scores"], out[f"py_{name}_in_cls"] = segs, scores, cls
        if mod is not None:
            t = [torch.from_numpy(x) for x in (segs, scores, cls)]
            ref = {k: tuple(x.numpy() for x in v) for k, v in case_runs(name, *t, mod.batched_nms).items()}
            for k in mine:
                assert same(ref[k][1], mine[k][1]) and same(ref[k][2], mine[k][2]), k
                assert np.allclose(ref[k][0], mine[k][0], rtol=1e-5, atol=0), k      # voted segments: the product's order differs
            mine = ref
        for k, (s, p, c) in mine.items():
            out[k + "_segs"], out[k + "_scores"], out[k + "_cls"] = s, p, c
            print(k, len(p))
    if mod is not None:
        e = mod.batched_nms(torch.zeros(0, 2), torch.zeros(0), torch.zeros(0, dtype=torch.int64), IOU, 0.0, MAX_SEG)
        assert [tuple(x.shape) for x in e] == [(0, 2), (0,), (0,)] and e[2].dtype == torch.int64 and e[0].dtype == torch.float32
    out["seeds"] = np.array(repr(sorted(seeds.items())))
    out["thresholds"] = np.array([IOU, SIGMA, VOTE])
    save("segnms", **out)


if __name__ == "__main__":
    main()
