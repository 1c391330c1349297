"""Development tool (GPU box): the launch list of the inference engine on the tiny configuration at batch 1, one line per
emitted launch: entry-point name and the stream it was emitted on (0 = main).  Two revisions that print the same list under
the same switches run the same kernels in the same order; the emitters are wrapped from outside, so one copy of this file
runs against any revision:   OTPOSE_CONV_MATH=f32 python tools/launch_list.py > list.txt"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from otpose_amd import OTPose, tiny_cfg                    # noqa: E402
from otpose_amd import synthetic as S                      # noqa: E402
from otpose_amd.engine import InferenceEngine              # noqa: E402

launches = []
call, call_lazy_nchw = InferenceEngine.call, InferenceEngine.call_lazy_nchw


def record_call(self, fn, name, *args):
    launches.append((name, self._sid))
    return call(self, fn, name, *args)


def record_call_lazy_nchw(self, aux, fn, name, *args, **kwargs):
    launches.append((name, self._sid))
    return call_lazy_nchw(self, aux, fn, name, *args, **kwargs)


InferenceEngine.call, InferenceEngine.call_lazy_nchw = record_call, record_call_lazy_nchw
model = S.fill_synthetic_(OTPose(tiny_cfg())).to("cuda:0").eval()
InferenceEngine(model, 1, "cuda:0", use_graph=False)
torch.cuda.synchronize()
for name, sid in launches:
    print(name, sid)
print(f"{len(launches)} launches", file=sys.stderr)
