"""GPU: ProgressiveViewHIP with every display stage on at once — the temporal carry, the
motion carry, the history trust and a filter — through the rt_render CLI, against the one restatement
of the view's display chain (tests/view_ref.py).  The tests of the single features (test_gpu_denoise,
_temporal, _variance, _motion, _trust, _sphere_motion) recompose through the same restatement, each
with its own flag, events and assertions.  Run on the MI355X box with `pytest -m gpu`."""
from __future__ import annotations

from dataclasses import replace

import numpy as np
import pytest

import view_ref as vr
from conftest import bits
from test_gpu_trust import TOL
from test_motion_host import small_move

pytestmark = pytest.mark.gpu

F = np.float32
W, H = 64, 48  # the smallest frame of the view tests: the a-trous step of 16 and the trust window have interior pixels
PX = W * H * 4
# displayed: progression 0, 1; the moved mesh's 1 (carried through the warp); the moved light's 1 (kept
# and judged); the new view's 1 and 2
EVENTS = "d,d,p:1,d,e:0.4:0:0,d,l,d,d"
N_SHOWN = 6
ALL_ON = vr.Flags(temporal=True, motion_carry=True, history_trust=True, tolerance=TOL)


@pytest.fixture(scope="module")
def mesh(pt):
    return pt.scenes.make_mesh(2000)  # rt_render --mesh 2000


@pytest.fixture(scope="module")
def rt(pt, mesh):
    t = pt.RayTracer(0)
    t.setSpheres(pt.scenes.ply_scene())
    t.setMesh(*mesh)
    yield t
    t.close()


@pytest.fixture(scope="module")
def poses(mesh):
    return np.stack([mesh[0], small_move(mesh[0])]).astype(F)


@pytest.fixture(scope="module")
def run(poses, tmp_path_factory):
    """flags -> that rt_render run's displayed, raw and feature frames; each flag set runs once."""
    tmp = tmp_path_factory.mktemp("view")
    poses.tofile(tmp / "poses.f32")
    cache = {}

    def get(flags):
        if flags not in cache:
            cache[flags] = vr.run_view(tmp, ["--mesh", "2000", "--poses", str(tmp / "poses.f32"), "--events", EVENTS] + flags.cli(),
                                       width=W, height=H)
        return cache[flags]

    return get


def frame(run, k):
    return run["shown"][PX * k:PX * (k + 1)]


@pytest.mark.parametrize("filter_flag", ["variance_guided", "denoise"])
def test_progressive_view_all_stages(filter_flag, run, rt, pt, mesh, poses):
    """--temporal --motion-carry --history-trust with --variance-guided, and with --denoise, over two
    displays, a mesh update, a display, a light move, a display, a key press and two displays.  Every
    displayed frame is the recomposition of momentsAccumulate / warpFeatures / reproject / historyTrust /
    temporalMerge / variance / denoiseVar / denoise that tests/view_ref.py makes from the run's raw
    frames, features, events and flags, bit for bit; the raw frames are those of the run without any
    display flag; and no flag is idle: the run without it (without --temporal: also without the two flags
    that need it) displays something else in at least one frame, and is its own recomposition too."""
    flags = replace(ALL_ON, **{filter_flag: True})
    on, plain = run(flags), run(vr.Flags())
    assert plain["shown"].size == N_SHOWN * PX and np.array_equal(bits(plain["shown"]), bits(plain["raw"]))
    assert [l["progression"] for l in on["lines"] if l.get("rendered")] == [0, 1, 1, 1, 1, 2]
    for fl in [flags] + [flags.without(name) for name in ("temporal", "motion_carry", "history_trust", filter_flag)]:
        got = run(fl)
        assert got["shown"].size == N_SHOWN * PX and got["feat"].size == 2 * N_SHOWN * PX
        assert np.array_equal(bits(got["raw"]), bits(plain["shown"])), fl
        exp = vr.displayed(rt, pt.scenes, fl, EVENTS, got["raw"], got["feat"], W, H, mesh=mesh, poses=poses).frames
        assert len(exp) == N_SHOWN
        for k in range(N_SHOWN):
            assert np.array_equal(bits(frame(got, k)), bits(exp[k])), f"{fl}: displayed frame {k}"
        if fl != flags:
            assert any(not np.array_equal(bits(frame(got, k)), bits(frame(on, k))) for k in range(N_SHOWN)), fl
