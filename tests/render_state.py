"""GPU tests' harness for "the render state is untouched": the golden progressive sequence of a triangle
case on a fresh tracer, what the sequence alone leaves behind, and the closing check that a second tracer
which made other calls in between left the same.  Each display stage's test_render_state_untouched
writes only its own calls between the renders, and its own assertions on what they gave."""
from __future__ import annotations

from contextlib import contextmanager

import numpy as np

from conftest import bits

CASE = "tris_64x48_sr1"


def tracer(pt, g, m):
    """A tracer set up as the golden case was rendered, counting."""
    t = pt.RayTracer(0)
    t.setSpheres(g["spheres"].view(pt._abi.SPHERE_DTYPE))
    t.setCamera(g["camera"])
    t.setSampleRate(m["sample_rate"])
    t.setMaxPathDepth(m["max_depth"])
    t.setNDRange(m["nd_y"])
    t.setMesh(g["verts"], g["idx"])
    t.setSeeds(m["Wpad"], m["Hpad"], g["seeds_in"])
    t.setCounting(True)
    return t


def totals(t):
    """The counter totals that count work: the clock readings, and the lane slots of the wave schedule,
    vary from one run of the same sequence to the next."""
    return {k: v for k, v in t.counterTotals().items() if "clocks" not in k and k != "lane_slots"}


def info(t):
    return {k: v for k, v in t.renderInfo().items() if k != "schedule_host_ms"}


@contextmanager
def untouched(pt, golden, golden_meta, compare_info=True):
    """Yields (t, frame, g, m): a fresh tracer on the golden case, the zeroed device frame, the case and
    its metadata.  The body renders the progressions 0 .. m["frames"] - 1 into `frame` with
    t.rayTrace(frame, W, H, p, kernel=2, sync=False) and makes its own calls in between; afterwards the
    device frame and rt_read are the golden last frame, and the seeds, the counter totals, the sign of
    the kernel time and the render info are those of the sequence alone, rendered first."""
    import torch

    g, m = golden(CASE), golden_meta["cases"][CASE]
    W, H = m["W"], m["H"]
    plain = tracer(pt, g, m)
    frame = torch.zeros(W * H * 4, dtype=torch.float32, device="cuda:0")
    for p in range(m["frames"]):
        plain.rayTrace(frame, W, H, p, kernel=2, sync=False)
    plain.synchronize()
    exp_totals, exp_seeds, exp_ms, exp_info = totals(plain), plain.getSeeds(), plain.lastKernelMs(), info(plain)
    assert np.array_equal(bits(frame.cpu().numpy()), bits(g["frames"][-1]))
    plain.close()

    t = tracer(pt, g, m)
    frame.zero_()
    try:
        yield t, frame, g, m
        t.synchronize()
        torch.cuda.synchronize()
        assert np.array_equal(bits(frame.cpu().numpy()), bits(g["frames"][-1]))
        back = np.zeros(W * H * 4, np.float32)
        t.read(back)
        assert np.array_equal(bits(back), bits(g["frames"][-1]))
        assert np.array_equal(t.getSeeds(), exp_seeds) and np.array_equal(exp_seeds, g["seeds_out"])
        got_totals = totals(t)
        assert got_totals == exp_totals and got_totals["renders"] == m["frames"] and got_totals["rays_closest"] > 0
        assert (t.lastKernelMs() > 0.0) == (exp_ms > 0.0)
        if compare_info:
            assert info(t) == exp_info
    finally:
        t.close()
