"""Development aid (GPU box): deformable PS-RoI pooling (csrc/deform_pool.hip) isolated at a detection-head size - 512 RoIs,
7x7 bins, group_size 7, out_channels 8, sample_per_part 4 on a (2, 392, 96, 72) map: time of the forward and of the backward
(workspace clear + bound + scatter + finish) and the bytes they have to move against the HBM peak."""
import os
import sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from otpose_amd import ops  # noqa: E402

HBM_PEAK = 8.0e12
n, c, h, w = 2, 392, 96, 72
rois_n, out_ch, g, pooled, part, spp, scale, tstd = 512, 8, 7, 7, 7, 4, 0.25, 0.1
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
gen = torch.Generator().manual_seed(0)
for dtype in (torch.float32, torch.float64):
    data = (torch.rand(n, c, h, w, generator=gen) * 2 - 1).to("cuda", dtype)
    x1, y1 = torch.rand(rois_n, generator=gen) * 4 * w * 0.7, torch.rand(rois_n, generator=gen) * 4 * h * 0.7
    bw, bh = 32 + torch.rand(rois_n, generator=gen) * 4 * w * 0.4, 32 + torch.rand(rois_n, generator=gen) * 4 * h * 0.4
    rois = torch.stack([torch.randint(0, n, (rois_n,), generator=gen).float(), x1, y1, x1 + bw, y1 + bh], 1).to("cuda", dtype)
    offset = (torch.rand(rois_n, 2, part, part, generator=gen) * 2 - 1).to("cuda", dtype)
    out, cnt = data.new_empty(rois_n, out_ch, pooled, pooled), data.new_empty(rois_n, out_ch, pooled, pooled)
    gout = torch.rand_like(out)
    gin, goff = torch.zeros_like(data), torch.zeros_like(offset)
    tail = (scale, out_ch, g, pooled, part, spp, tstd)
    esz = data.element_size()
    samples = rois_n * out_ch * pooled * pooled * spp * spp
    for no_trans in (False, True):
        fwd = lambda: ops.deform_psroi_pooling_cuda_forward(data, rois, offset, out, cnt, no_trans, *tail)   # noqa: E731
        bwd = lambda: ops.deform_psroi_pooling_cuda_backward(gout, data, rois, offset, cnt, gin, goff, no_trans, *tail)   # noqa: E731
        # compulsory traffic: the forward reads the map once and writes out + count; the backward clears and reads back the 8-byte
        # plane, reads and writes grad_input, and reads the map again for the offset gradient.  Gathered: 4 neighbours per sample.
        plane = n * c * h * w
        fbytes = plane * esz + 2 * out.numel() * esz
        bbytes = plane * (8 + 8 + 2 * esz) + (0 if no_trans else plane * esz) + 2 * out.numel() * esz
        for name, f, byts, gathered in (("forward", fwd, fbytes, samples * 4 * esz), ("backward", bwd, bbytes, samples * 4 * 8)):
            for _ in range(3):
                f()
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                f()
            b.record()
            torch.cuda.synchronize()
            t = a.elapsed_time(b) / reps * 1e-3
            print("%s %s no_trans=%d: %.1f us | compulsory %.1f MB -> %.0f GB/s = %.1f %% of the %.1f TB/s HBM peak | gathered / "
                  "scattered %.1f MB -> %.0f GB/s | valid samples %.0f %%"
                  % (str(dtype).split(".")[1], name, no_trans, t * 1e6, byts / 1e6, byts / t / 1e9, 100 * byts / t / HBM_PEAK,
                     HBM_PEAK / 1e12, gathered / 1e6, gathered / t / 1e9, 100 * float(cnt.sum()) / samples), flush=True)
