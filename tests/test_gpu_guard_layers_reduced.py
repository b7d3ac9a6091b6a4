"""Where svc_hip_decode_layers_reduced_frames writes and what its result depends on (tests/helpers/guarded.py): rec, display, status
and the doubled workspace of exactly the sizes the API asks for inside guarded allocations, the four poisons, and other bytes beside each
of its five inputs.  The streams are those of tests/test_gpu_decode_layers_reduced.py."""
import numpy as np
import pytest
import torch

from scalable_video_codec_amd import native as nat
from tests.helpers import guarded as gd
from tests.test_gpu_decode_layers_reduced import N_FRAMES, _pair
from tests.test_gpu_decode_levels import _rects

pytestmark = pytest.mark.gpu

U8, I32, F32 = torch.uint8, torch.int32, torch.float32


@pytest.mark.parametrize("block,reduce", [(8, 2), (16, 8)])
def test_layered_reduced_decode_writes_inside_its_buffers_and_reads_only_its_inputs(native, block, reduce):
    n, w, h, mv = N_FRAMES, 336, 48, 16  # full groups plus a partial one at both tile sizes
    p = _pair(w, h, block, mv, (4, 16, 1), "cut")
    rw, rh = w // reduce, h // reduce
    dw, dh = rw - 5, rh - 3
    gaze = torch.from_numpy(np.asarray(_rects(n, w, h), dtype=np.uint32).view(np.int32).reshape(n, 4)).cuda()
    assert nat.decode_layers_reduced_workspace_bytes(n, w, h, block) == 2 * nat.decode_levels_workspace_bytes(n, w, h, block)
    written = {"workspace": gd.Guarded(nat.decode_layers_reduced_workspace_bytes(n, w, h, block), U8, "cuda", seed=0),
               "rec": gd.Guarded(n * rh * rw * 3 * 4, F32, "cuda", seed=1, shape=(n, rh, rw, 3)),
               "display": gd.Guarded(n * dh * dw * 3, U8, "cuda", seed=2, shape=(n, dh, dw, 3)),
               "status": gd.Guarded(n * 4, I32, "cuda", seed=3)}
    ws, rec, disp, status = (written[k].interior for k in ("workspace", "rec", "display", "status"))

    def call(inputs, **kw):
        # (the binding allocates its own status: the raw entry point, so that status too is the guarded one)
        steps = kw.get("steps", (3, 17))
        g = inputs["gaze"] if kw.get("with_gaze", True) else None
        nat._check(nat.load().svc_hip_decode_layers_reduced_frames(
            inputs["base"].data_ptr(), inputs["base"].numel(), inputs["base offsets"].data_ptr(), inputs["enhancement"].data_ptr(),
            inputs["enhancement"].numel(), inputs["enhancement offsets"].data_ptr(), n, w, h, block, block, mv, mv, *steps, reduce,
            None if g is None else g.data_ptr(), ws.data_ptr(), ws.numel(), rec.data_ptr(), disp.data_ptr(), dw, dh, status.data_ptr(),
            nat._stream()))
        torch.cuda.synchronize()
        assert status.cpu().tolist() == [0] * n
        return {"rec": rec, "display": disp, "status": status}

    given = {"base": p.base, "base offsets": p.base_offs, "enhancement": p.enh, "enhancement offsets": p.enh_offs, "gaze": gaze}
    # the dirty call: other steps and no gaze, which is the one-stream route on the first half of the workspace
    findings = gd.check_writes("decode_layers_reduced", written, lambda: call(given),
                               dirty=lambda: call(given, steps=(7, 9), with_gaze=False), seed=block)
    findings += gd.check_reads("decode_layers_reduced", given, call, written)
    assert not findings, "\n".join(findings)
    assert rec.abs().max().item() > 1  # a picture, not zeros
