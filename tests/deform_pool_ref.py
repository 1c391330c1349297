"""Plain numpy reference of deformable position-sensitive RoI pooling, forward and backward, written from the operator's
description (include/otpose_hip.h); the yardstick of tests/test_deform_pool_host.py and tests/test_gpu_deform_pool.py.  It
imports nothing from otpose_amd.

Every coordinate step is carried out in ``ctype`` (float64 by default, float32 for the tests' estimate of what float32
coordinates cost); values, weights' products and sums are always float64.  RoI corners are rounded half AWAY from zero as C's
round() does - numpy's round (half to even) is not used anywhere.
"""
import math

import numpy as np


def round_half_away(x):
    """C round(): nearest integer, halves away from zero."""
    x = float(x)
    return math.copysign(math.floor(abs(x) + 0.5), x)


def _clampi(v, lo, hi):
    return lo if v < lo else (hi if v > hi else v)


def _geometry(data, offset, no_trans, out_channels, group_size):
    n, c, h, w = data.shape
    assert c == out_channels * group_size * group_size
    if no_trans:
        return 1, out_channels
    assert offset.shape[1] % 2 == 0
    num_classes = offset.shape[1] // 2
    assert out_channels % num_classes == 0
    return num_classes, out_channels // num_classes


def _samples(data_shape, rois, offset, no_trans, spatial_scale, out_channels, group_size, out_size, part_size, sample_per_part,
             trans_std, ctype, num_classes, cec):
    """Yield, per output element, (n, ctop, ph, pw, batch, c, cls, part_h, part_w, roi_w, roi_h, [(w, h) of every sample]) with
    the coordinates BEFORE the skip test and the clamp, computed step by step in ``ctype``."""
    T = ctype
    _, _, H, W = data_shape
    half, one = T(0.5), T(1)
    for n in range(rois.shape[0]):
        r = rois[n]
        batch = int(r[0])
        sw = T(T(round_half_away(r[1])) * T(spatial_scale)) - half
        sh = T(T(round_half_away(r[2])) * T(spatial_scale)) - half
        ew = T(T(T(round_half_away(r[3])) + one) * T(spatial_scale)) - half
        eh = T(T(T(round_half_away(r[4])) + one) * T(spatial_scale)) - half
        roi_w = max(T(ew - sw), T(0.1))
        roi_h = max(T(eh - sh), T(0.1))
        bin_w, bin_h = T(roi_w / T(out_size)), T(roi_h / T(out_size))
        sub_w, sub_h = T(bin_w / T(sample_per_part)), T(bin_h / T(sample_per_part))
        for ctop in range(out_channels):
            cls = ctop // cec
            for ph in range(out_size):
                for pw in range(out_size):
                    part_h = int(math.floor(T(T(T(ph) / T(out_size)) * T(part_size))))
                    part_w = int(math.floor(T(T(T(pw) / T(out_size)) * T(part_size))))
                    gh = _clampi(int(math.floor(T(T(T(ph) * T(group_size)) / T(out_size)))), 0, group_size - 1)
                    gw = _clampi(int(math.floor(T(T(T(pw) * T(group_size)) / T(out_size)))), 0, group_size - 1)
                    if no_trans:
                        tx = ty = T(0)
                    else:
                        tx = T(T(offset[n, 2 * cls, part_h, part_w]) * T(trans_std))
                        ty = T(T(offset[n, 2 * cls + 1, part_h, part_w]) * T(trans_std))
                    wstart = T(T(T(pw) * bin_w) + sw)
                    wstart = T(wstart + T(tx * roi_w))
                    hstart = T(T(T(ph) * bin_h) + sh)
                    hstart = T(hstart + T(ty * roi_h))
                    pts = []
                    for ih in range(sample_per_part):
                        for iw in range(sample_per_part):
                            pts.append((T(wstart + T(T(iw) * sub_w)), T(hstart + T(T(ih) * sub_h))))
                    c = (ctop * group_size + gh) * group_size + gw
                    yield n, ctop, ph, pw, batch, c, cls, part_h, part_w, roi_w, roi_h, pts


def _tap(w, h, W, H, T):
    """None for a skipped sample, else (x0, x1, y0, y1, dx, dy) of the clamped sample."""
    if w < -0.5 or w > W - 0.5 or h < -0.5 or h > H - 0.5:
        return None
    w = min(max(w, T(0)), T(W - 1))
    h = min(max(h, T(0)), T(H - 1))
    x0, x1, y0, y1 = int(math.floor(w)), int(math.ceil(w)), int(math.floor(h)), int(math.ceil(h))
    return x0, x1, y0, y1, T(w - T(x0)), T(h - T(y0))


def forward(data, rois, offset, no_trans, spatial_scale, out_channels, group_size, out_size, part_size, sample_per_part,
            trans_std, ctype=np.float64):
    """Returns (output, output_count) as float64 arrays of shape (num_rois, out_channels, out_size, out_size)."""
    data = np.asarray(data, np.float64)
    rois = np.asarray(rois, np.float64)
    offset = None if no_trans else np.asarray(offset, np.float64)
    num_classes, cec = _geometry(data, offset, no_trans, out_channels, group_size)
    H, W = data.shape[2:]
    out = np.zeros((rois.shape[0], out_channels, out_size, out_size))
    cnt = np.zeros_like(out)
    for n, ctop, ph, pw, batch, c, _, _, _, _, _, pts in _samples(
            data.shape, rois, offset, no_trans, spatial_scale, out_channels, group_size, out_size, part_size, sample_per_part,
            trans_std, ctype, num_classes, cec):
        plane = data[batch, c]
        total, k = 0.0, 0
        for w, h in pts:
            t = _tap(w, h, W, H, ctype)
            if t is None:
                continue
            x0, x1, y0, y1, dx, dy = t
            dx, dy = float(dx), float(dy)
            total += ((1 - dx) * (1 - dy) * plane[y0, x0] + (1 - dx) * dy * plane[y1, x0]
                      + dx * (1 - dy) * plane[y0, x1] + dx * dy * plane[y1, x1])
            k += 1
        out[n, ctop, ph, pw] = total / k if k else 0.0
        cnt[n, ctop, ph, pw] = k
    return out, cnt


def backward(grad_out, data, rois, offset, output_count, no_trans, spatial_scale, out_channels, group_size, out_size, part_size,
             sample_per_part, trans_std, ctype=np.float64):
    """Returns (grad_input, grad_offset): the contributions alone (the operator adds them to its caller's buffers).
    grad_offset is None with ``no_trans``.  Elements with output_count <= 0 contribute nothing."""
    data = np.asarray(data, np.float64)
    rois = np.asarray(rois, np.float64)
    grad_out = np.asarray(grad_out, np.float64)
    offset = None if no_trans else np.asarray(offset, np.float64)
    num_classes, cec = _geometry(data, offset, no_trans, out_channels, group_size)
    H, W = data.shape[2:]
    gin = np.zeros_like(data)
    goff = None if no_trans else np.zeros_like(offset)
    for n, ctop, ph, pw, batch, c, cls, part_h, part_w, roi_w, roi_h, pts in _samples(
            data.shape, rois, offset, no_trans, spatial_scale, out_channels, group_size, out_size, part_size, sample_per_part,
            trans_std, ctype, num_classes, cec):
        k = output_count[n, ctop, ph, pw]
        if k <= 0:
            continue
        diff = grad_out[n, ctop, ph, pw] / k
        plane = data[batch, c]
        for w, h in pts:
            t = _tap(w, h, W, H, ctype)
            if t is None:
                continue
            x0, x1, y0, y1, dx, dy = t
            dx, dy = float(dx), float(dy)
            gin[batch, c, y0, x0] += (1 - dx) * (1 - dy) * diff
            gin[batch, c, y1, x0] += (1 - dx) * dy * diff
            gin[batch, c, y0, x1] += dx * (1 - dy) * diff
            gin[batch, c, y1, x1] += dx * dy * diff
            if no_trans:
                continue
            u00, u01, u10, u11 = plane[y0, x0], plane[y1, x0], plane[y0, x1], plane[y1, x1]
            gx = (u11 * dy + u10 * (1 - dy) - u01 * dy - u00 * (1 - dy)) * trans_std * diff * float(roi_w)
            gy = (u11 * dx + u01 * (1 - dx) - u10 * dx - u00 * (1 - dx)) * trans_std * diff * float(roi_h)
            goff[n, 2 * cls, part_h, part_w] += gx
            goff[n, 2 * cls + 1, part_h, part_w] += gy
    return gin, goff


def min_guard_distance(data_shape, rois, offset, no_trans, spatial_scale, out_channels, group_size, out_size, part_size,
                       sample_per_part, trans_std):
    """Smallest distance (fp64 coordinates) of any sample coordinate from a line where the operator is discontinuous or
    kinked: the integer grid lines (which include the clamp edges 0, W-1, H-1) and the skip borders -0.5, W-0.5, H-0.5."""
    _, _, H, W = data_shape
    rois = np.asarray(rois, np.float64)
    offset = None if no_trans else np.asarray(offset, np.float64)
    num_classes = 1 if no_trans else offset.shape[1] // 2
    best = np.inf
    for item in _samples(data_shape, rois, offset, no_trans, spatial_scale, out_channels, group_size, out_size, part_size,
                         sample_per_part, trans_std, np.float64, num_classes, out_channels // num_classes):
        for w, h in item[-1]:
            for v, size in ((float(w), W), (float(h), H)):
                best = min(best, abs(v - round_half_away(v)), abs(v + 0.5), abs(v - (size - 0.5)), abs(v), abs(v - (size - 1)))
    return best


# the six RoIs every case holds, for a (2, C, 9, 7) map at a spatial_scale near 0.9: (batch, x1, y1, x2, y2)
BASE_ROIS = np.array([
    [0, 1.2, 1.7, 4.3, 6.1],        # inside the map
    [0, 3.8, 5.2, 11.1, 13.3],      # hangs over the right and bottom borders: some bins count fewer than spp^2 samples
    [0, 20.2, 30.1, 24.3, 33.2],    # entirely outside: count 0, output 0, no gradient
    [0, 4.1, 2.2, 1.3, 5.4],        # x2 < x1: the 0.1 minimum width applies
    [0, 0.5, 1.5, 3.5, 4.5],        # .5 corners: round() takes them away from zero (0.5 -> 1, 1.5 -> 2, 3.5 -> 4, 4.5 -> 5)
    [1, 0.9, 2.1, 5.2, 7.8],        # batch index 1
], np.float64)

GUARD = 1e-3
MAX_DRAWS = 200


def guarded_case(seed, out_size, group_size, part_size, sample_per_part, num_classes, no_trans, trans_std=0.1,
                 map_hw=(9, 7), batch=2, channels_per_class=2):
    """Draw (data, rois, offset, grad_out, kwargs) for one configuration, REJECTING draws in which any sample coordinate lies
    within GUARD of a discontinuity (min_guard_distance): such a sample may legitimately fall on the other side in float32.
    A condition on the inputs, not a tolerance.
    The RoIs are BASE_ROIS with corners jittered by less than 0.2 (never across a .5, so the rounding is the base's; the .5
    RoI is kept as it is); spatial_scale is drawn from [0.85, 0.95] (without offsets the samples depend on nothing else: at
    scale 1 many of them sit exactly on grid lines); offsets are uniform in [-1, 1], data and grad_out in [-1, 1].
    spatial_scale and trans_std are rounded to float32, the type in which the operator's interface carries them.
    Asserts a draw is accepted within MAX_DRAWS."""
    out_channels = channels_per_class * num_classes
    H, W = map_hw
    C = out_channels * group_size * group_size
    trans_std = float(np.float32(trans_std))
    rng = np.random.RandomState(seed)
    for draw in range(MAX_DRAWS):
        spatial_scale = float(np.float32(rng.uniform(0.85, 0.95)))
        rois = BASE_ROIS.copy()
        jitter = rng.uniform(-0.15, 0.15, size=(rois.shape[0], 4))
        jitter[4] = 0.0
        rois[:, 1:] += jitter
        offset = rng.uniform(-1.0, 1.0, size=(rois.shape[0], 2 * num_classes, part_size, part_size))
        args = (rois, None if no_trans else offset, bool(no_trans), spatial_scale, out_channels, group_size, out_size, part_size,
                sample_per_part, trans_std)
        if min_guard_distance((batch, C, H, W), *args) > GUARD:
            data = rng.uniform(-1.0, 1.0, size=(batch, C, H, W))
            grad_out = rng.uniform(-1.0, 1.0, size=(rois.shape[0], out_channels, out_size, out_size))
            kw = dict(no_trans=bool(no_trans), spatial_scale=spatial_scale, out_channels=out_channels, group_size=group_size,
                      out_size=out_size, part_size=part_size, sample_per_part=sample_per_part, trans_std=trans_std)
            return data, rois, offset, grad_out, kw
    raise AssertionError(f"no guarded draw within {MAX_DRAWS} for out_size {out_size}, group_size {group_size}, part_size "
                         f"{part_size}, sample_per_part {sample_per_part}, {num_classes} classes, no_trans {no_trans}")
