"""The weight-EMA update restated in numpy from its formula (include/otpose_hip.h, "weight EMA"):

    ema <- decay * ema + (1 - decay) * model

with ``decay`` and ``1 - decay`` (the subtraction in double) each rounded to float32 once, the two products and the sum each
rounded to float32 - three operations, no fused multiply-add - and, for an int64 entry, both operands converted to float32 first
and the float32 result converted back by truncation toward zero.  tests/test_ema_host.py holds this to tests/golden/ema.npz (the
reference class on the CPU); the GPU tests hold the kernels to the same file."""
import numpy as np

STATES = 5
DECAYS = (0.999, 0.9, 0.0)


def scalars(decay):
    """(float32(decay), float32(1.0 - decay)) as the host passes them to the kernels."""
    return np.float32(decay), np.float32(1.0 - float(decay))


def ema_update(ema, model, decay):
    """One update of one tensor; returns an array of ``ema``'s dtype (float32 or int64)."""
    d, omd = scalars(decay)
    e = np.asarray(ema).astype(np.float32)
    m = np.asarray(model).astype(np.float32)
    with np.errstate(all="ignore"):
        a = np.multiply(d, e, dtype=np.float32)
        b = np.multiply(omd, m, dtype=np.float32)
        r = np.add(a, b, dtype=np.float32)
    if np.asarray(ema).dtype == np.int64:
        return np.trunc(r).astype(np.int64)
    return r


def load(z):
    """(keys, start, [src1..src5], {decay: [ema after call 1..5]}) of the arrays of ema.npz, each state a dict key -> array."""
    keys = [k[len("start/"):] for k in z if k.startswith("start/")]
    start = {k: np.asarray(z["start/" + k]) for k in keys}
    srcs = [{k: np.asarray(z[f"src{i}/{k}"]) for k in keys} for i in range(1, STATES + 1)]
    emas = {d: [{k: np.asarray(z[f"ema_{d}_{i}/{k}"]) for k in keys} for i in range(1, STATES + 1)] for d in DECAYS}
    return keys, start, srcs, emas


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    view = np.uint32 if a.dtype == np.float32 else np.int64
    return bool(np.array_equal(a.reshape(-1).view(view), b.reshape(-1).view(view)))
