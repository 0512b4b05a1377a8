"""The torch hand-over of Context.pack_tensor (tests/test_gpu_tensor.py starts this as a process of its own): torch is imported
first and the library after it, as bench.py imports them.  An out= tensor of torch.float16 and one of torch.bfloat16 on the
device equal torch.from_numpy of the reference under torch.equal, and the call downloads nothing.  Prints TORCH_HAND_OVER_OK."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import librectify_amd as L  # noqa: E402
import numpy_tensor_ref as ref  # noqa: E402
from test_gpu_tensor import IMAGENET_MEAN, IMAGENET_STD, PIX_U8X3, picture, spec_kwargs  # noqa: E402


def main():
    assert torch.cuda.is_available()
    dev = torch.device("cuda", 0)
    ctx = L.Context(0)
    pics = [picture(130, 33, 3, 1), picture(65, 17, 3, 2), picture(1, 1, 3, 3)]
    for dtype, tdtype in (("f16", torch.float16), ("bf16", torch.bfloat16)):
        for layout in ("nchw", "nhwc"):
            spec = L.TensorSpec((33, 131), dtype, layout, mean=IMAGENET_MEAN, std=IMAGENET_STD, pad=(3, 120, 255))
            out = torch.full(spec.shape(3, PIX_U8X3), -7.0, dtype=tdtype, device=dev)
            torch.cuda.synchronize()
            calls = []
            real = ctx.device_download
            ctx.device_download = lambda *a, **k: calls.append(a) or real(*a, **k)
            try:
                back = ctx.pack_tensor(pics, spec, out=out)
            finally:
                del ctx.device_download
            assert back is out and not calls
            kw = spec_kwargs(L, spec, PIX_U8X3)
            want = np.stack([ref.slot(p, *ref.place((33, 131), (p.shape[1], p.shape[0])), **kw) for p in pics])
            want_t = torch.from_numpy(want.view(np.int16)).view(torch.bfloat16) if dtype == "bf16" else torch.from_numpy(want)
            assert torch.equal(out.cpu(), want_t), (dtype, layout)
            assert torch.equal(out, want_t.to(dev)), (dtype, layout)
    spec = L.TensorSpec((33, 131), "f16")
    for wrong in (torch.empty((3, 3, 33, 131), dtype=torch.float32, device=dev), torch.empty((2, 3, 33, 131), dtype=torch.float16, device=dev),
                  torch.empty((3, 3, 33, 262), dtype=torch.float16, device=dev)[..., ::2], torch.empty((3, 3, 33, 131), dtype=torch.float16)):
        try:
            ctx.pack_tensor(pics, spec, out=wrong)
        except ValueError:
            continue
        raise AssertionError("an out= of the wrong dtype, shape, layout or device was taken")
    ctx.close()
    print("TORCH_HAND_OVER_OK")


if __name__ == "__main__":
    main()
