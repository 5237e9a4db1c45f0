"""The inline list resolve of the triangle megakernel: a new sample's camera ray is
tested against the first RT_INLINE_LIST records of its pixel's candidate list where the ray is made
(k_tris phase B) instead of in the stepping loop, and the lanes it answers take a further pass of the
path advance in the same iteration (RT_INLINE_CHAIN bounds those passes).  The same float tests run
on the same records in the same order with the same accept rule and early end, so frames, both seed
planes and the three ray counts must not move by a bit, whatever K and the bound.  Both knobs are
read at every render.
"""
from __future__ import annotations

import numpy as np
import pytest

from conftest import bits

pytestmark = pytest.mark.gpu

RAYS = ("rays_closest", "rays_shadow", "rays_skipped")
KNOBS = ("RT_INLINE_LIST", "RT_INLINE_CHAIN", "RT_LIST_MB", "RT_PIXEL_LISTS", "RT_SPLIT", "RTMI_GRID_BLOCKS")
KS = ("0", "1", "2", "3")
W, H, SR = 64, 48, 4


def _camera(sc, w, distance=None, azimuth=None):
    c = dict(sc.PLY_CAMERA)
    if distance is not None:
        c["distance"] = distance
    if azimuth is not None:
        c["azimuth"] = azimuth
    return sc.camera_spherical(w, **c)


def _render(pt, mp, env, verts, idx, cams, w=W, h=H, sr=SR, tile=None, counting=False, skip=7):
    """One fresh context under `env`; `cams` is a list of (camera, progressions): every frame is
    rendered in turn.  Returns (bits of the last frame, seeds, ray counts per frame, list counts of
    the last frame, render info, counters of the last frame)."""
    for k in KNOBS:
        mp.delenv(k, raising=False)
    mp.setenv("RT_PIXEL_LISTS", "1")  # lists on whatever the frame's size
    for k, v in env.items():
        mp.setenv(k, v)
    sc = pt.scenes
    Wp, Hp = sc.padded_dims(w, h)
    rt = pt.RayTracer(0)
    rt.setSpheres(sc.ply_scene())
    rt.setSampleRate(sr)
    rt.setMaxPathDepth(6)
    rt.setMesh(verts, idx)
    rt.setSeeds(Wp, Hp, sc.default_seeds(Wp, Hp, skip=skip))
    if counting:
        rt.setCounting(True)
    rows = h if tile is None else int(((np.arange(h) // tile[0]) % tile[1] == tile[2]).sum())
    got = np.zeros(rows * w * 4, np.float32)
    rays = []
    for cam, progs in cams:
        rt.setCamera(cam)
        for p in progs:
            rt.rayTrace(got, w, h, p, kernel=2, tile=tile)
            c = rt.counters()
            rays.append(tuple(c[k] for k in RAYS))
    out = (bits(got).copy(), rt.getSeeds().copy(), rays, rt.listCounts().copy(), rt.renderInfo(), c)
    rt.close()
    return out


def _oracle(pt, oracle, verts, idx, cams, w=W, h=H, sr=SR, skip=7):
    """The same frames by the oracle's BVH mode: (frame bits, seeds, (closest, shadow) per frame)."""
    sc = pt.scenes
    Wp, Hp = sc.padded_dims(w, h)
    sd = sc.default_seeds(Wp, Hp, skip=skip)
    exp = np.zeros(w * h * 4, np.float32)
    bvh = oracle.build_bvh(verts, idx)
    counts = []
    for cam, progs in cams:
        for p in progs:
            counts.append(tuple(oracle.render_tris(exp, cam, sc.ply_scene(), w, h, Wp, Hp, sr, 6, p, sd, verts, idx,
                                                   bvh=bvh)))
    bvh.close()
    return bits(exp).copy(), sd, counts


def _vs_oracle(got, exp, what):
    np.testing.assert_array_equal(got[0], exp[0], err_msg=f"{what}: frame")
    np.testing.assert_array_equal(got[1], exp[1], err_msg=f"{what}: seeds")
    assert [r[:2] for r in got[2]] == [tuple(c[:2]) for c in exp[2]], (what, got[2], exp[2])


def _same(a, b, what):
    np.testing.assert_array_equal(a[0], b[0], err_msg=f"{what}: frame")
    np.testing.assert_array_equal(a[1], b[1], err_msg=f"{what}: seeds")
    assert a[2] == b[2], f"{what}: ray counts {a[2]} != {b[2]}"


@pytest.fixture(scope="module")
def mesh2k(pt):
    """The golden fixtures' triangle mesh (tests/golden/meta.json: rt_make_mesh(2000))."""
    return pt.scenes.make_mesh(2000)


@pytest.fixture(scope="module")
def close_view(pt, oracle, mesh2k):
    """The mesh filling the 64x48 frame (distance 3.2): every pixel has a list, short and long ones."""
    cams = [(_camera(pt.scenes, W, distance=3.2), (0,))]
    return cams, _oracle(pt, oracle, *mesh2k, cams)


@pytest.fixture(scope="module")
def far_view(pt, oracle, mesh2k):
    """The mesh inside the frame (distance 5): pixels with empty lists and box paths around it."""
    cams = [(_camera(pt.scenes, W), (0,))]
    return cams, _oracle(pt, oracle, *mesh2k, cams)


@pytest.fixture(scope="module")
def far_k0(pt, mesh2k, far_view):
    mp = pytest.MonkeyPatch()
    try:
        return _render(pt, mp, {"RT_INLINE_LIST": "0"}, *mesh2k, far_view[0])
    finally:
        mp.undo()


def test_view_has_every_list_length(far_k0):
    """The far view holds lists of 1, 2, 3 and 4 records (a list of exactly K and of K + 1 records
    for each K tested: walked to its end inline, or handed over with one record left), lists inside
    the first block beyond every K, and lists of more than 8 records (later blocks on the stack), so
    the cases below do not pass vacuously; around the mesh it has empty-list pixels, whose box paths
    share their waves with the listed pixels.  The lengths are the render's own list codes."""
    n = far_k0[3]
    assert n.size == W * H and far_k0[4]["lists"] == 1
    assert (n == 0).any() and far_k0[2][0][2] > 0  # empty lists; queries answered without a traversal
    hist = np.bincount(n[n != 0xFFFF].astype(np.int64), minlength=66)
    print("list lengths 0..12:", hist[:13].tolist(), "over 8:", int(hist[9:].sum()), "tree:", int((n == 0xFFFF).sum()))
    for length in (1, 2, 3, 4):
        assert hist[length] > 0, (length, hist[:13].tolist())
    assert hist[5:9].sum() > 0 and hist[9:].sum() > 0, hist[:13].tolist()


@pytest.mark.parametrize("k", KS)
def test_far_view_vs_oracle(pt, monkeypatch, mesh2k, far_view, far_k0, k):
    cams, exp = far_view
    for chain in ("0", "1", "2"):
        got = _render(pt, monkeypatch, {"RT_INLINE_LIST": k, "RT_INLINE_CHAIN": chain}, *mesh2k, cams)
        _vs_oracle(got, exp, f"K {k} chain {chain}")
        _same(got, far_k0, f"K {k} chain {chain} against K 0")


def test_default_knobs(pt, monkeypatch, mesh2k, far_view, far_k0):
    got = _render(pt, monkeypatch, {}, *mesh2k, far_view[0])
    _vs_oracle(got, far_view[1], "defaults")
    _same(got, far_k0, "defaults against K 0")


@pytest.mark.parametrize("k", KS)
def test_tree_pixels_beside_listed_ones(pt, monkeypatch, mesh2k, close_view, k):
    """A list area too small for every pixel (RT_LIST_MB=1: the pixels that do not fit take the tree,
    RT_LPACK_NONE) on the close view, whose every pixel has candidates."""
    cams, exp = close_view
    got = _render(pt, monkeypatch, {"RT_INLINE_LIST": k, "RT_LIST_MB": "1"}, *mesh2k, cams)
    n = got[3]
    assert (n == 0xFFFF).any() and ((n > 0) & (n != 0xFFFF)).any(), np.unique(n)
    assert got[4]["list_pixels_tree"] == int((n == 0xFFFF).sum())
    _vs_oracle(got, exp, f"small list area, K {k}")


def test_lane_takes_pixel_after_pixel(pt, monkeypatch, mesh2k, far_view):
    """One block of 256 lanes for the frame's 3072 pixels (RTMI_GRID_BLOCKS=1): every lane takes a
    dozen pixels in turn, each with its own list word.  (rays_skipped is compared on this grid: how
    many box-path queries are answered without a traversal follows the frame's launch form.)"""
    cams, exp = far_view
    base = None
    for k in KS:
        got = _render(pt, monkeypatch, {"RT_INLINE_LIST": k, "RTMI_GRID_BLOCKS": "1"}, *mesh2k, cams)
        assert got[4]["grid_blocks"] == 1
        _vs_oracle(got, exp, f"one block, K {k}")
        base = base or got
        _same(got, base, f"one block, K {k} against K 0")


def test_progressive_frames_and_camera_move(pt, oracle, monkeypatch, mesh2k):
    """Three progressive frames of one view (the second and third reuse its lists), then a frame after
    a camera move (the lists are rebuilt)."""
    sc = pt.scenes
    cams = [(_camera(sc, W, distance=3.2), (0, 1, 2)), (_camera(sc, W, distance=3.4, azimuth=80.0), (0,))]
    exp = _oracle(pt, oracle, *mesh2k, cams)
    base = None
    for k in KS:
        got = _render(pt, monkeypatch, {"RT_INLINE_LIST": k}, *mesh2k, cams)
        assert got[4]["lists"] == 1 and got[4]["lists_rebuilt"] == 1
        _vs_oracle(got, exp, f"progressive, K {k}")
        base = base or got
        _same(got, base, f"progressive, K {k} against K 0")


def test_sample_split_tile(pt, oracle, monkeypatch, mesh2k):
    """One 8-way row-stripe tile of the close view at sampleRate 16 through the sample-split path
    (RT_SPLIT=1: chunk tasks take the same phase B): the tile's rows of the oracle's frame, and every
    K against K = 0."""
    sc = pt.scenes
    sr, tile = 16, (8, 8, 3)
    cams = [(_camera(sc, W, distance=3.2), (0,))]
    exp = _oracle(pt, oracle, *mesh2k, cams, sr=sr)
    rows = np.flatnonzero((np.arange(H) // tile[0]) % tile[1] == tile[2])
    exp_rows = exp[0].reshape(H, W * 4)[rows].ravel()
    base = None
    for k in KS:
        got = _render(pt, monkeypatch, {"RT_INLINE_LIST": k, "RT_SPLIT": "1"}, *mesh2k, cams, sr=sr, tile=tile)
        assert got[4]["split_chunks"] > 0, got[4]
        np.testing.assert_array_equal(got[0], exp_rows, err_msg=f"split tile, K {k}")
        base = base or got
        _same(got, base, f"split tile, K {k} against K 0")


def test_counting_launch(pt, monkeypatch, mesh2k, far_view, far_k0):
    """A counting launch: the inline tests are counted as the loop's are, and both walk the same
    records (a query ends at the same record wherever it is tested), so tris_tested, leaves_visited
    and nodes_visited are K = 0's; the frame and the three ray counts are the plain launch's."""
    cams, exp = far_view
    base = None
    for k in KS:
        got = _render(pt, monkeypatch, {"RT_INLINE_LIST": k}, *mesh2k, cams, counting=True)
        print(f"K {k}: rays {got[2]}, plain launch {far_k0[2]}")
        _same(got, far_k0, f"counting, K {k}")
        c = {f: got[5][f] for f in ("tris_tested", "leaves_visited", "nodes_visited") + RAYS}
        print(f"K {k}: {c}, lane_slots {got[5]['lane_slots']}")
        assert c["tris_tested"] > 0
        base = base or c
        assert c == base, (k, c, base)
