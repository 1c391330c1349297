#!/usr/bin/env python
"""Development measurement of the weight EMA (otpose_amd/ema.py, csrc/optim.hip) at the W48 384x288 configuration; the
numbers of DESIGN.md section 0 come from here.  Needs the MI355X.

    python tools/ema_bench.py [--batch 16] [--reps 50] [--steps 7] [--no-train-step] [--out FILE.json]

(a) ``ModelEma.update`` as built, over the full ``state_dict()`` of a model whose trainable parameters live in FusedAdamW's flat
    buffer: device time per call (events around ``reps`` back-to-back calls), host time per call (enqueue only), and the host
    cost of the moved-storage check alone;
(b) the reference's per-tensor loop (thirdparty/utils/train_utils.py:251-259) run by PyTorch ops on the same device;
(c) the bf16 training step of bench.py's probe (same model, inputs, optimizer) with and without ``ema=``, alternating, every
    step synchronised, median of ``steps`` each;
(d) ``otp_ema_update`` alone on the flat buffer against the HBM peak (12 bytes per element: two reads, one write), next to
    ``otp_axpby`` and to one table job over the same buffers.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from otpose_amd import ModelEma, OTPose, cfg2, hip, parallel as PAR       # noqa: E402
from otpose_amd import synthetic as S                                      # noqa: E402
from otpose_amd.optim import FusedAdamW                                    # noqa: E402

HBM_PEAK = 8.0e12            # bytes/s, MI355X


def device_ms(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    host = (time.perf_counter() - t0) / reps
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps, 1e3 * host


def reference_loop(ema_module, model, decay):
    with torch.no_grad():
        for ema_v, model_v in zip(ema_module.state_dict().values(), model.state_dict().values()):
            ema_v.copy_(decay * ema_v + (1. - decay) * model_v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--no-train-step", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ema_bench.py measures on the MI355X; there is no CPU path")
    dev = torch.device("cuda", 0)
    cfg = cfg2()
    model = OTPose(cfg)
    S.fill_synthetic_(model)
    model = model.to(dev).train()
    model.train_dtype = "bf16"
    opt = FusedAdamW([p for p in model.parameters() if p.requires_grad], lr=1e-4, weight_decay=0.01, max_grad_norm=1.0)
    ema = ModelEma(model, decay=0.999)
    ema.update(model)
    plan = ema._plan
    sd = model.state_dict()
    elements = sum(v.numel() for v in sd.values())
    res = {"config": "cfg2 (W48, 384x288)", "state_dict_entries": len(sd), "state_dict_elements": elements,
           "flat_elements": plan["single"][2] if plan["single"] else 0, "table_jobs": plan["n_jobs"]}

    # (a)
    dms, hms = device_ms(lambda: ema.update(model), a.reps)
    t0 = time.perf_counter()
    for _ in range(a.reps):
        ema._current_plan(model)
    check_ms = 1e3 * (time.perf_counter() - t0) / a.reps
    res["a_model_ema_update"] = {"device_ms": dms, "host_ms": hms, "moved_storage_check_host_ms": check_ms, "launches": int(
        plan["single"] is not None) + int(plan["n_jobs"] > 0)}

    # (b)
    ref_copy = ModelEma(model, decay=0.999).module
    dms_b, hms_b = device_ms(lambda: reference_loop(ref_copy, model, 0.999), max(3, a.reps // 10), warmup=1)
    res["b_reference_loop_torch_ops"] = {"device_ms": dms_b, "host_ms": hms_b}
    del ref_copy

    # (d)
    if plan["single"]:
        mirror, src_ptr, n = plan["single"]
        L = hip.lib()
        src = opt._flat[0]["p"]
        assert src.data_ptr() == src_ptr and src.numel() == n
        scratch = torch.empty_like(mirror)
        d, omd = 0.999, float(1. - 0.999)
        job = ctypes.create_string_buffer(L.otp_ema_job_bytes())
        hip.check(L.otp_ema_job(hip.ptr(scratch), hip.ptr(src), n, hip.CONSTANTS["OTP_DTYPE_F32"], None, job), "otp_ema_job")
        table = torch.frombuffer(bytearray(job.raw), dtype=torch.uint8).to(dev)
        runs = {"otp_ema_update": lambda: L.otp_ema_update(hip.ptr(scratch), hip.ptr(src), n, d, omd, hip.stream_of(src)),
                "otp_axpby": lambda: L.otp_axpby(hip.ptr(src), hip.ptr(scratch), omd, d, n, hip.stream_of(src)),
                "otp_ema_update_table_one_job": lambda: L.otp_ema_update_table(hip.ptr(table), 1, d, omd, hip.stream_of(src))}
        scratch.copy_(mirror)
        flat = {k: [] for k in runs}
        for _ in range(3):                                       # alternating, three rounds
            for k, fn in runs.items():
                flat[k].append(device_ms(fn, a.reps)[0])
        res["d_flat_pass"] = {k: {"device_ms": sorted(v)[1], "rounds_ms": v, "bytes": 12 * n,
                                  "bytes_per_s": 12 * n / (1e-3 * sorted(v)[1]), "frac_of_hbm_peak": 12 * n / (1e-3 * sorted(v)[1]) / HBM_PEAK}
                              for k, v in flat.items()}
        del scratch

    # (c)
    if not a.no_train_step:
        x, margin = S.synthetic_clip(a.batch, cfg.MODEL.IMAGE_SIZE)
        x, margin = x.to(dev), margin.to(dev)
        J = cfg.MODEL.NUM_JOINTS
        w, h = cfg.MODEL.HEATMAP_SIZE
        gen = torch.Generator().manual_seed(11)
        g = (torch.rand(a.batch, J, h, w, generator=gen) * 0.2).to(dev)
        g[:, ::2, 3, 4] = 1.0
        wt = (torch.rand(a.batch, J, 1, generator=gen) > 0.15).float().to(dev)
        times = {False: [], True: []}
        for it in range(2 * (a.steps + 1)):
            with_ema = bool(it & 1)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            PAR.train_step_dp(model, opt, x, margin, g, wt, ema=ema if with_ema else None)
            torch.cuda.synchronize()
            if it >= 2:
                times[with_ema].append(1e3 * (time.perf_counter() - t0))
        med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
        res["c_train_step_bf16"] = {"batch": a.batch, "ms_per_step_without_ema": med[False], "ms_per_step_with_ema": med[True],
                                    "all_ms_without": times[False], "all_ms_with": times[True]}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
