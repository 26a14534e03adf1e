"""A frame WITH the post filter captured once as a HIP graph and replayed: with
a median-fill launch budget (sgm_set_post_filter_launches) the post filter
enqueues a fixed launch sequence and reads nothing back, so the map the
reference's get_disp() returns can be replayed like every other output.  Each
replay must give the eager adaptive map and the oracle's, bit for bit, and
check() after each replay must find the fill proven.  (Without a budget the
capture is refused: test_gpu_graph.py::test_capture_with_post_filter_is_rejected.)"""
from __future__ import annotations

import numpy as np
import pytest
import torch

import oracle
from support import f32_bits as bits
from stereo_matching_amd import SGM, synthetic

pytestmark = pytest.mark.gpu


@pytest.mark.timeout(120)
@pytest.mark.parametrize("h,w,D,views,sky,slant,lk", [
    (96, 320, 64, 2, False, False, False),
    (120, 256, 128, 2, True, False, False),
    (96, 320, 64, 2, False, True, False),       # the slanted passes (SGM_SLANT=1)
    (96, 320, 64, 2, False, False, True),       # + LKRefine, fed from the filter's staging map
])
def test_post_filtered_frame_replays_from_a_hip_graph(h, w, D, views, sky, slant, lk, monkeypatch):
    monkeypatch.setenv("SGM_SLANT", "1" if slant else "0")
    dev = torch.device("cuda", 0)
    budget = -(-w // 64) * h + 1       # always proves the fill (DESIGN.md "Post filter")
    mask = synthetic.sky_mask(h, w) if sky else None
    with SGM(h, w, 1, D, views=views, post_filter=True, lk_refine=lk,
             post_filter_launches=budget) as sgm, \
            SGM(h, w, 1, D, views=views, post_filter=True, lk_refine=lk) as adaptive:
        stream = torch.cuda.ExternalStream(sgm.stream, device=dev)
        d_l = torch.empty((h, w), dtype=torch.uint8, device=dev)
        d_r = torch.empty_like(d_l)
        d_sky = torch.from_numpy(mask).to(dev) if sky else None
        skyp = d_sky.data_ptr() if sky else 0
        out_e = torch.empty((h, w), dtype=torch.float32, device=dev)
        out_g = torch.empty_like(out_e)

        def frame(handle, out, st):
            handle.process_device(d_l.data_ptr(), d_r.data_ptr(), out.data_ptr(), d_sky_l=skyp,
                                  d_sky_r=skyp if views == 2 else 0, stream=st)

        def load(k):
            left, right = synthetic.stereo_pair(h, w, D, pair_index=k)
            with torch.cuda.stream(stream):
                d_l.copy_(torch.from_numpy(left))
                d_r.copy_(torch.from_numpy(right))
            return left, right

        load(0)
        with torch.cuda.stream(stream):
            frame(sgm, out_g, stream.cuda_stream)  # warm-up (the capture needs no first-call work)
        torch.cuda.synchronize(dev)
        sgm.check()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream, capture_error_mode="relaxed"):
            frame(sgm, out_g, stream.cuda_stream)
        torch.cuda.synchronize(dev)
        for k in (1, 2, 3):
            left, right = load(k)
            with torch.cuda.stream(stream):
                graph.replay()
            torch.cuda.synchronize(dev)
            sgm.check()                            # the replayed fill was proven
            assert 1 <= sgm.post_filter_proved_at() <= budget
            g = out_g.cpu().numpy()
            # the eager adaptive map of the same buffers (the stream is idle: ordered by the sync)
            frame(adaptive, out_e, None)
            adaptive.check()
            e = out_e.cpu().numpy()
            want = oracle.process(left, right, D, sky_l=mask, sky_r=mask)["final"]
            if lk:
                want = oracle.lk_refine(left, right, want, D)
            assert np.array_equal(bits(g), bits(e)), k
            assert np.array_equal(bits(g), bits(want)), k
