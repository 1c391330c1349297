#!/usr/bin/env python
"""Generate tests/golden/lr_schedule.json by running the reference's ``make_scheduler`` (build container only).

Run from the repo root:  ``python tests/golden/make_optim_golden.py``

The four branches of thirdparty/utils/train_utils.py:140-205 (TRAIN.WARMUP true / false x TRAIN.LR_SCHEDULER in
CosineAnnealingLR / MultiStepLR) over three parameter groups with the base rates of ``make_optimizer``'s groups
(LR, LR, LR / 100), stepped once per iteration as script/Common.py:143-144 does.  Stored: ``group["lr"]`` of every group at
17 consecutive iterations as float64 - two more than ``max_steps`` of the warm-up branches, so the periodic branch of the
warm-up cosine (lr_schedulers.py:91) is in the table.
"""
from __future__ import annotations

import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from otpose_amd.config import CfgNode                          # noqa: E402
from tests.golden.make_golden import import_reference          # noqa: E402

TRAIN = {"WARMUP_EPOCHS": 2, "END_EPOCH": 3, "EPOCHS": 5, "GAMMA": 0.1}
ITERS_PER_EPOCH = 3
BASE_LRS = [1e-4, 1e-4, 1e-6]
ITERATIONS = 17


def main():
    import_reference()
    from thirdparty.utils.train_utils import make_scheduler
    branches = {}
    for warmup in (True, False):
        for name in ("CosineAnnealingLR", "MultiStepLR"):
            cfg = CfgNode({"TRAIN": dict(TRAIN, WARMUP=warmup, LR_SCHEDULER=name)})
            params = [torch.nn.Parameter(torch.zeros(2)) for _ in BASE_LRS]
            opt = torch.optim.SGD([{"params": [p], "lr": lr} for p, lr in zip(params, BASE_LRS)], lr=BASE_LRS[0])
            sched = make_scheduler(opt, cfg, ITERS_PER_EPOCH)
            table = [[] for _ in BASE_LRS]
            for _ in range(ITERATIONS):
                for row, g in zip(table, opt.param_groups):
                    row.append(float(g["lr"]))
                opt.step()
                sched.step()
            branches[("warmup_" if warmup else "plain_") + name] = table
    out = {"train": TRAIN, "iters_per_epoch": ITERS_PER_EPOCH, "base_lrs": BASE_LRS, "iterations": ITERATIONS,
           "lr": branches}
    path = os.path.join(HERE, "lr_schedule.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", path)
    for k, v in branches.items():
        print(" ", k, " ".join("%.4g" % x for x in v[0]))


if __name__ == "__main__":
    main()
