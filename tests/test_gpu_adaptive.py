"""GPU: adaptive sampling on the noise meter's tile map.  Masked raytrace_tris renders
against the oracle — the expected state after each call is select(mask, oracle(state), state), every word
of the framebuffer and of both seed planes; the masked order kernel alone; the stop rule and the masked
moments against tests/adaptive_ref.py, bit for bit; and ProgressiveViewHIP::setAdaptive through the
rt_render CLI.  Run on the MI355X box with `pytest -m gpu`."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import adaptive_ref as ar
import render_state as rs
import view_ref as vr
from conftest import bits

pytestmark = pytest.mark.gpu

CASE = "tris_64x48_sr1"
F = np.float32
U = np.uint32
SIZES = [(8, 8), (37, 29), (64, 48)]


def device(a):
    import torch

    return torch.from_numpy(a.view(np.int32) if a.dtype == U else a).cuda()


def host(t):
    a = t.cpu().numpy()
    return a.view(U) if a.dtype == np.int32 else a


@pytest.fixture(scope="module")
def scene(pt, oracle, golden, golden_meta):
    """The golden triangle scene, and the oracle's render of it at any size."""
    from oracle import MeshBVH

    g, m = golden(CASE), golden_meta["cases"][CASE]
    sc = pt.scenes
    spheres = g["spheres"].view(pt._abi.SPHERE_DTYPE)
    bvh = MeshBVH(oracle, g["verts"], g["idx"])

    def render(acc, W, H, sr, progression, seeds):
        Wp, Hp = sc.padded_dims(W, H)
        return oracle.render_tris(acc, sc.camera_spherical(W, **sc.PLY_CAMERA), spheres, W, H, Wp, Hp, sr, m["max_depth"],
                                  progression, seeds, g["verts"], g["idx"], bvh=bvh)

    def tracer(W, H, sr, traversal="bvh", counting=False):
        t = pt.RayTracer(0)
        t.setSpheres(spheres)
        t.setCamera(sc.camera_spherical(W, **sc.PLY_CAMERA))
        t.setSampleRate(sr)
        t.setMaxPathDepth(m["max_depth"])
        t.setMesh(g["verts"], g["idx"])
        t.setTraversal(traversal)
        t.setCounting(counting)
        return t

    return dict(render=render, tracer=tracer, sc=sc)


def masks(W, H, seed=0):
    """The planes of a W x H frame by name (0 = live; stopped tiles carry different words)."""
    tw, th = ar.tile_grid(W, H)
    n = tw * th
    ty, tx = np.divmod(np.arange(n), tw)
    rng = np.random.default_rng(100 * W + H + seed)
    words = rng.integers(1, 1 << 31, n).astype(U)
    words[0] = U(0xFFFFFFFF)
    live = dict(all=np.ones(n, bool), none=np.zeros(n, bool), one=np.arange(n) == n // 2,
                edges=((tx == tw - 1) & (W % 8 != 0)) | ((ty == th - 1) & (H % 8 != 0)), checker=(tx + ty) % 2 == 0,
                random=rng.random(n) < 0.5)
    return {k: np.where(v, U(0), words).astype(U) for k, v in live.items()}


class Masked:
    """A tracer rendering progressive frames into a device frame under a borrowed device plane, beside the
    expected state: select(mask, oracle(state), state)."""

    def __init__(self, scene, W, H, sr, traversal="bvh", counting=False, seed_skip=7):
        import torch

        sc = scene["sc"]
        self.scene, self.W, self.H, self.sr = scene, W, H, sr
        self.Wp, self.Hp = sc.padded_dims(W, H)
        self.t = scene["tracer"](W, H, sr, traversal, counting)
        self.seeds = sc.default_seeds(self.Wp, self.Hp, skip=seed_skip).copy()
        self.t.setSeeds(self.Wp, self.Hp, self.seeds)
        # (no zeros: a stopped tile keeps what the frame held, whatever that was)
        self.exp = np.random.default_rng(W + H).random(W * H * 4).astype(F)
        self.frame = device(self.exp)
        self.plane = torch.zeros(ar.n_tiles(W, H), dtype=torch.int32, device="cuda:0")
        self.on = False

    def close(self):
        self.t.close()

    def render(self, progression, mask):
        """One frame under `mask` (None: the plane cleared), checked word for word; returns the counters."""
        import torch

        W, H = self.W, self.H
        if mask is None:
            self.t.setTileStop(None)
            self.on = False
        else:
            self.plane.copy_(device(mask))  # changed through the borrowed pointer
            torch.cuda.synchronize()
            if not self.on:
                self.t.setTileStop(self.plane, W, H)
                self.on = True
        self.t.rayTrace(self.frame, W, H, progression, kernel=2)
        full, seeds_full = self.exp.copy(), self.seeds.copy()
        self.scene["render"](full, W, H, self.sr, progression, seeds_full)
        stop = np.zeros(ar.n_tiles(W, H), U) if mask is None else mask
        self.exp, self.seeds = ar.masked(stop, W, H, self.Wp, self.Hp, self.exp, full, self.seeds, seeds_full)
        what = (W, H, self.sr, progression)
        np.testing.assert_array_equal(bits(host(self.frame)), bits(self.exp), err_msg=f"frame {what}")
        np.testing.assert_array_equal(self.t.getSeeds(), self.seeds, err_msg=f"seeds {what}")
        return self.t.counters()

    def restore(self, frame, seeds):
        self.exp, self.seeds = frame.copy(), seeds.copy()
        self.frame.copy_(device(self.exp))
        self.t.setSeeds(self.Wp, self.Hp, self.seeds)


SEQUENCES = [("random", "checker", "all"), ("one", "edges", "none")]


@pytest.mark.parametrize("sr", [1, 2])
@pytest.mark.parametrize("W,H", SIZES)
def test_masked_render_equals_selected_oracle(scene, W, H, sr):
    """Three progressive frames under planes changed in between (not monotone), then the plane cleared and
    an unmasked frame: the oracle again."""
    mk = masks(W, H)
    for names in SEQUENCES:
        m = Masked(scene, W, H, sr)
        try:
            for p, name in enumerate(names):
                m.render(p, mk[name])
                info = m.t.renderInfo()
                assert info["split_chunks"] == 0 and info["schedule_pilot"] == 0 and info["schedule_measured"] == 0, info
            assert m.t.lastAdaptiveMs(order=True) > 0.0
            m.render(3, None)
        finally:
            m.close()


@pytest.mark.parametrize("traversal", ["bvh4f", "linear"])
@pytest.mark.parametrize("W,H", SIZES)
def test_masked_render_identity_order(scene, W, H, traversal):
    """The traversals without a schedule: the masked order is compacted from the identity."""
    mk = masks(W, H, seed=1)
    m = Masked(scene, W, H, 1, traversal)
    try:
        for p, name in enumerate(("checker", "random", "edges")):
            m.render(p, mk[name])
        m.render(3, None)
    finally:
        m.close()


@pytest.mark.parametrize("W,H", SIZES)
def test_masked_frame_after_a_sample_split_frame(scene, W, H):
    """sampleRate 4: the unmasked first frame is sample-split at these sizes; the masked frame after it is a
    whole-pixel launch that reuses the split frame's order and classes."""
    mk = masks(W, H, seed=2)
    m = Masked(scene, W, H, 4)
    try:
        m.render(0, None)
        assert m.t.renderInfo()["split_chunks"] > 0
        m.render(1, mk["random"])
        info = m.t.renderInfo()
        assert info["split_chunks"] == 0 and info["pixels_long"] == 0, info
        m.render(2, mk["checker"])
    finally:
        m.close()


WORK = ("rays_closest", "rays_shadow", "nodes_visited", "tris_tested", "leaves_visited", "rays_skipped", "pixel_rays_max",
        "pixel_steps_max")


@pytest.mark.parametrize("counting", [True, False])
def test_counters_of_masked_renders(scene, counting):
    """From one state: all live counts what the unmasked frame counts; none traces no ray and changes no
    word; the rays of a mask and of its complement sum to the frame's."""
    W, H = 37, 29
    mk = masks(W, H, seed=3)
    m = Masked(scene, W, H, 1, counting=counting)
    try:
        m.render(0, None)
        m.render(1, mk["all"])  # (the view's lists exist from here on)
        frame0, seeds0 = m.exp.copy(), m.seeds.copy()
        got = {}
        for name, mask in (("full", None), ("all", mk["all"]), ("none", mk["none"]), ("a", mk["random"]),
                           ("not_a", np.where(mk["random"] == 0, U(3), U(0)).astype(U))):
            m.restore(frame0, seeds0)
            got[name] = m.render(2, mask)
        keys = WORK if counting else WORK[:2]
        assert {k: got["all"][k] for k in keys} == {k: got["full"][k] for k in keys} and got["full"]["rays_closest"] > 0
        assert got["none"]["rays_closest"] == 0 and got["none"]["rays_shadow"] == 0
        for k in WORK[:2]:
            assert got["a"][k] + got["not_a"][k] == got["full"][k] and 0 < got["a"][k] < got["full"][k], k
        # (none: Masked.render compared every word of the frame and of the seeds with the state before it)
    finally:
        m.close()


def test_render_argument_checks(pt, scene):
    """While a plane is set, a render it cannot mask is an error with a message, never a full render."""
    import torch

    ab = pt._abi
    W, H = 37, 29
    m = Masked(scene, W, H, 1)
    try:
        m.render(0, masks(W, H)["checker"])
        t = m.t
        before = host(m.frame).copy()
        seeds = t.getSeeds()
        other = torch.zeros(64 * 48 * 4, dtype=torch.float32, device="cuda:0")
        for kw, buf in ((dict(kernel=0), m.frame), (dict(kernel=1), m.frame), (dict(kernel=2, tile=(8, 2, 0)), m.frame),
                        (dict(kernel=2, width=64, height=48), other), (dict(kernel=2, width=29, height=37), m.frame)):
            w, h = kw.pop("width", W), kw.pop("height", H)
            with pytest.raises(ab.RtError) as e:
                t.rayTrace(buf, w, h, 1, **kw)
            assert e.value.status == ab.RT_ERR_ARG and "stop plane" in str(e.value), (kw, str(e.value))
        assert np.array_equal(bits(host(m.frame)), bits(before)) and np.array_equal(t.getSeeds(), seeds) and not other.any()
        lib, p = t._lib, ab.ptr
        plane = np.zeros(ar.n_tiles(W, H), U)
        for args in ((p(plane), W, H, 2), (p(plane), 0, H, 0), (p(plane), W, 0, 0), (p(plane), 1 << 14, 1 << 14, 0)):
            assert lib.rt_set_tile_stop(t._h, *args) == ab.RT_ERR_ARG and lib.rt_last_error(t._h)
        m.render(1, masks(W, H)["random"])  # the plane set before still holds
        # a host plane is copied at the call: changing the array afterwards changes nothing
        plane[:] = masks(W, H)["one"]
        t.setTileStop(plane, W, H)
        mask = plane.copy()
        plane[:] = 0
        m.on = True
        t.rayTrace(m.frame, W, H, 2, kernel=2)
        full, seeds_full = m.exp.copy(), m.seeds.copy()
        scene["render"](full, W, H, 1, 2, seeds_full)
        exp, exp_seeds = ar.masked(mask, W, H, m.Wp, m.Hp, m.exp, full, m.seeds, seeds_full)
        assert np.array_equal(bits(host(m.frame)), bits(exp)) and np.array_equal(t.getSeeds(), exp_seeds)
        t.setTileStop(None)
        t.rayTrace(other, 64, 48, 0, kernel=2)  # cleared: any size again
    finally:
        m.close()


# ---- the masked order kernel alone --------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 7, 48, 4097, 70000])
def test_order_kernel(tracer, n):
    """Random base permutations and the identity, planes from all live to none: stable, exactly n entries,
    each at most n, and the live count; host arrays and device tensors."""
    rng = np.random.default_rng(n)
    for k, share in enumerate((0.0, 0.4, 0.97, 1.0)):
        stop = ((rng.random(n) < share) * rng.integers(1, 1 << 32, n)).astype(U)
        for base in (None, rng.permutation(n).astype(U)):
            exp, live = ar.order(base, stop)
            out, cnt = np.full(n, 0xDEADBEEF, U), np.full(1, 0xDEADBEEF, U)
            tracer.tileStopOrder(base, stop, out, cnt)
            assert np.array_equal(out, exp) and cnt[0] == live, (n, share, base is None)
            d_out, d_cnt = device(np.full(n + 1, 0xDEADBEEF, U)), device(np.full(1, 0xDEADBEEF, U))
            tracer.tileStopOrder(None if base is None else device(base), device(stop), d_out, d_cnt)
            got = host(d_out)
            assert np.array_equal(got[:n], exp) and got[n] == 0xDEADBEEF and host(d_cnt)[0] == live  # exactly n entries
    assert tracer.lastAdaptiveMs(order=True) > 0.0
    bad = np.array([n + 5] + list(range(1, n)), U)  # an entry that is no tile index counts as stopped
    exp, live = ar.order(bad, np.zeros(n, U))
    out, cnt = np.zeros(n, U), np.zeros(1, U)
    tracer.tileStopOrder(bad, np.zeros(n, U), out, cnt)
    assert np.array_equal(out, exp) and cnt[0] == live == n - 1


# ---- the stop rule and the masked moments -------------------------------------------------------

SHAPES = [(1, 1), (7, 5), (64, 48), (300, 200)]


def tile_maps(W, H, seed):
    """(mean, max) pairs around the default thresholds, with the odd values a map can hold."""
    n = ar.n_tiles(W, H)
    rng = np.random.default_rng(seed)
    t = np.empty((n, 2), F)
    t[:, 0] = np.exp(rng.normal(np.log(0.05), 0.7, n))
    t[:, 1] = t[:, 0] * rng.uniform(1.0, 8.0, n)
    odd = np.array([[0.05, 0.2], [np.nextafter(F(0.05), F(1)), 0.2], [0.05, np.nextafter(F(0.2), F(1))], [0, 0], [np.nan, 0],
                    [0, np.nan], [0.01, np.inf], [-0.0, -0.0]], F)
    k = min(len(odd), n)
    t[rng.permutation(n)[:k]] = odd[:k]
    return t


@pytest.mark.parametrize("W,H", SHAPES)
def test_select_equals_numpy(tracer, W, H):
    n = ar.n_tiles(W, H)
    rng = np.random.default_rng(W)
    for seed, prm in enumerate((dict(), dict(dilate=0), dict(dilate=4, min_frames=3), dict(max_ratio=np.inf, dilate=2),
                                dict(threshold=0.0), dict(min_frames=99))):
        tiles = tile_maps(W, H, seed)
        stop = ((rng.random(n) < 0.3) * rng.integers(1, 40, n)).astype(U)
        exp, exp_st = ar.select(tiles, stop, 17, W, H, **{**ar.DEFAULTS, **prm})
        got = stop.copy()
        st = tracer.tileStopSelect(tiles, got, 17, W, H, **prm)
        assert np.array_equal(got, exp) and st == exp_st, (prm, st, exp_st)
        d_stop, d_tiles = device(stop), device(tiles)
        st = tracer.tileStopSelect(d_tiles, d_stop, 17, W, H, **prm)
        assert np.array_equal(host(d_stop), exp) and st == exp_st and np.array_equal(bits(host(d_tiles)), bits(tiles))
    assert tracer.lastAdaptiveMs() > 0.0
    with pytest.raises(ValueError):
        tracer.tileStopSelect(tiles, device(stop), 17, W, H)  # host and device buffers mixed


def test_select_on_hand_made_planes(tracer):
    """The planes of tests/test_adaptive_host.py through the kernels: a noisy tile's ring at dilate 0, 1 and
    4, a corner, a stopped neighbour, decisions from the old plane, and a monotone sequence of calls."""
    W, H = 72, 56
    tw, th = ar.tile_grid(W, H)
    for at in ((3, 4), (0, 0), (th - 1, tw - 1)):
        t = np.full((th, tw, 2), 0.01, F)
        t[at] = (1.0, 1.0)
        for d in (0, 1, 4):
            exp, exp_st = ar.select(t, np.zeros(tw * th, U), 16, W, H, dilate=d)
            got = np.zeros(tw * th, U)
            assert tracer.tileStopSelect(t.reshape(-1), got, 16, W, H, dilate=d) == exp_st and np.array_equal(got, exp)
    for tiles, stop in (([[1, 1], [0.01, 0.01], [0.01, 0.01]], [5, 0, 0]), ([[0.01, 0.01], [1, 1], [0.01, 0.01]], [0, 0, 0]),
                        ([[9, 9]] * 3, [3, 0, 8])):
        tiles, stop = np.array(tiles, F), np.array(stop, U)
        exp, exp_st = ar.select(tiles, stop, 16, 24, 8, dilate=1)
        assert tracer.tileStopSelect(tiles, stop, 16, 24, 8, dilate=1) == exp_st and np.array_equal(stop, exp)
    rng = np.random.default_rng(8)
    stop, ref = device(np.zeros(tw * th, U)), np.zeros(tw * th, U)
    for n in range(1, 12):
        t = tile_maps(W, H, 50 + n)
        ref, exp_st = ar.select(t, ref, n, W, H, min_frames=4, dilate=1)
        assert tracer.tileStopSelect(device(t), stop, n, W, H, min_frames=4, dilate=1) == exp_st
        assert np.array_equal(host(stop), ref)
    assert (ref != 0).any() and (ref == 0).any()


def frames(W, H, seed):
    rng = np.random.default_rng(seed)
    prev = np.exp(rng.normal(-1.0, 1.0, W * H * 4)).astype(F)
    cur = (prev + rng.normal(0.0, 0.05, W * H * 4)).astype(F)  # some recovered samples are negative
    mom = rng.random(W * H * 4).astype(F)
    n = ar.n_tiles(W, H)
    stop = ((rng.random(n) < 0.5) * rng.integers(1, 100, n)).astype(U)
    return prev, cur, mom, stop


@pytest.mark.parametrize("W,H", SHAPES)
def test_masked_moments_equal_numpy(tracer, W, H):
    """Host arrays and device tensors, in place and into another buffer, n_cur 1 (with and without mom_in)
    and 7; live tiles are momentsAccumulate's bits, the inputs are only read."""
    px = W * H
    for seed in (0, 1):
        prev, cur, mom, stop = frames(W, H, seed)
        for n in (7.0, 1.0):
            exp, exp_len = ar.moments_tiles(prev, cur, n, mom, stop, W, H)
            plain = np.zeros(4 * px, F)
            tracer.momentsAccumulate(prev, cur, n, mom, plain, W, H)
            live = np.repeat(ar.pixel_mask(stop, W, H), 4)
            assert np.array_equal(bits(plain)[live], bits(exp)[live])  # one copy of the arithmetic
            for dev in (False, True):
                wrap = device if dev else (lambda a: a.copy())
                a = [wrap(x) for x in (prev, cur, mom, stop)]
                out, ln = wrap(np.full(4 * px, 5.0, F)), wrap(np.full(px, -1.0, F))
                tracer.momentsAccumulateTiles(a[0], a[1], n, a[2], out, a[3], ln, W, H)
                back = (lambda t: host(t)) if dev else (lambda t: t)
                assert np.array_equal(bits(back(out)), bits(exp)) and np.array_equal(bits(back(ln)), bits(exp_len)), (seed, n, dev)
                for got, src in zip(a, (prev, cur, mom, stop)):
                    assert np.array_equal(bits(back(got)), bits(src))
                tracer.momentsAccumulateTiles(a[0], a[1], n, a[2], a[2], a[3], ln, W, H)  # in place
                assert np.array_equal(bits(back(a[2])), bits(exp)) and np.array_equal(bits(back(ln)), bits(exp_len))
        # the view's first frame: no history; a stopped tile keeps what the output held
        keep = np.full(4 * px, 5.0, F)
        exp, exp_len = ar.moments_tiles(None, cur, 1.0, None, stop, W, H, mom_out=keep)
        for dev in (False, True):
            out, ln = (device(keep), device(np.zeros(px, F))) if dev else (keep.copy(), np.zeros(px, F))
            tracer.momentsAccumulateTiles(None, device(cur) if dev else cur, 1.0, None, out, device(stop) if dev else stop, ln, W, H)
            assert np.array_equal(bits(host(out) if dev else out), bits(exp)) and np.array_equal(bits(host(ln) if dev else ln), bits(exp_len))
    assert tracer.lastVarianceMs("moments") > 0.0


def test_argument_checks(pt, tracer):
    ab = pt._abi
    lib, p = tracer._lib, ab.ptr
    W, H = 20, 9  # 3 x 2 tiles
    n = ar.n_tiles(W, H)
    tiles, stop, stats = tile_maps(W, H, 1).reshape(-1), np.zeros(n, U), np.zeros(4, U)
    nan, inf = float("nan"), float("inf")

    def select(tl_=tiles, sp_=stop, n_=16, st_=stats, w_=W, h_=H, prm=(0.05, 4.0, 16, 1), flags=0):
        pr = ab.RtAdaptiveParams(*prm) if prm else None
        return lib.rt_tile_stop_select(tracer._h, p(tl_), p(sp_), n_, p(st_), w_, h_, ctypes.byref(pr) if pr else None, flags)

    assert select() == ab.RT_OK and select(prm=(0.0, 1.0, 0, 0)) == ab.RT_OK and select(prm=(3e38, inf, 1, 4)) == ab.RT_OK
    stop[:] = 0
    stats[:] = 0
    for kw in (dict(tl_=None), dict(sp_=None), dict(st_=None), dict(prm=None), dict(n_=0), dict(w_=0), dict(h_=0),
               dict(w_=1 << 14, h_=1 << 14), dict(flags=2), dict(prm=(-0.1, 4.0, 16, 1)), dict(prm=(nan, 4.0, 16, 1)),
               dict(prm=(0.05, 0.5, 16, 1)), dict(prm=(0.05, nan, 16, 1)), dict(prm=(0.05, 4.0, 16, 5)),
               dict(sp_=tiles.view(U)), dict(sp_=tiles.view(U)[4:]), dict(st_=stop), dict(st_=tiles.view(U)[2:])):
        assert select(**kw) == ab.RT_ERR_ARG, {k: type(v) for k, v in kw.items()}
        assert lib.rt_last_error(tracer._h)
    assert not stop.any() and not stats.any()

    prev, cur, mom, plane = frames(W, H, 3)
    out, ln = np.zeros(4 * W * H, F), np.zeros(W * H, F)

    def moments(pv_=prev, cu_=cur, n_=7.0, mi_=mom, mo_=out, sp_=plane, ln_=ln, w_=W, h_=H, flags=0):
        return lib.rt_moments_accumulate_tiles(tracer._h, p(pv_), p(cu_), n_, p(mi_), p(mo_), p(sp_), p(ln_), w_, h_, flags)

    assert moments() == ab.RT_OK and moments(pv_=None, mi_=None, n_=1.0) == ab.RT_OK
    for kw in (dict(cu_=None), dict(mo_=None), dict(sp_=None), dict(ln_=None), dict(pv_=None), dict(mi_=None), dict(n_=0.5),
               dict(n_=nan), dict(w_=0), dict(flags=2), dict(mo_=cur), dict(mo_=prev), dict(ln_=mom), dict(ln_=out[8:]),
               dict(ln_=plane.view(F)), dict(sp_=out.view(U)[4:])):
        assert moments(**kw) == ab.RT_ERR_ARG, {k: type(v) for k, v in kw.items()}
        assert lib.rt_last_error(tracer._h)

    order, live = np.zeros(n, U), np.zeros(1, U)

    def make_order(bs_=None, sp_=plane, n_=n, od_=order, lv_=live, flags=0):
        return lib.rt_tile_stop_order(tracer._h, p(bs_), p(sp_), n_, p(od_), p(lv_), flags)

    assert make_order() == ab.RT_OK
    for kw in (dict(sp_=None), dict(od_=None), dict(lv_=None), dict(n_=0), dict(n_=1 << 28), dict(flags=2), dict(od_=plane),
               dict(lv_=plane[2:]), dict(lv_=order[1:]), dict(bs_=order)):
        assert make_order(**kw) == ab.RT_ERR_ARG, {k: type(v) for k, v in kw.items()}
    t = pt.RayTracer(0)
    try:
        ms = ctypes.c_float()
        assert t._lib.rt_last_adaptive_ms(t._h, ctypes.byref(ms), None) == ab.RT_ERR_STATE
        assert t._lib.rt_last_adaptive_ms(t._h, None, ctypes.byref(ms)) == ab.RT_ERR_STATE
        assert t._lib.rt_last_adaptive_ms(t._h, None, None) == ab.RT_ERR_ARG
    finally:
        t.close()


def test_render_state_untouched(pt, golden, golden_meta):
    """The golden progressive frames with the stop rule, the masked moments and the order kernel in between
    — device tensors on a side stream behind a render enqueued without a wait, host buffers on the context's
    stream — are the frames, seeds, counter totals, render info and rt_read of the sequence without them."""
    import torch

    with rs.untouched(pt, golden, golden_meta) as (t, frame_dev, g, m):
        W, H = m["W"], m["H"]
        n = ar.n_tiles(W, H)
        tiles = tile_maps(W, H, 4)
        prev, cur, mom, plane = frames(W, H, 5)
        exp_stop, exp_st = ar.select(tiles, plane, 20, W, H, **{**ar.DEFAULTS, "dilate": 0})
        exp_mom, exp_len = ar.moments_tiles(prev, cur, 6.0, mom, plane, W, H)
        exp_order, exp_live = ar.order(None, plane)
        d_tiles, d_prev, d_cur, d_mom = (device(a) for a in (tiles, prev, cur, mom))
        per = range(m["frames"])
        d_stop = [device(plane) for _ in per]
        d_stats = [torch.zeros(4, dtype=torch.int32, device="cuda:0") for _ in per]
        d_out = [torch.zeros(4 * W * H, dtype=torch.float32, device="cuda:0") for _ in per]
        d_len = [torch.zeros(W * H, dtype=torch.float32, device="cuda:0") for _ in per]
        d_ord = [torch.zeros(n, dtype=torch.int32, device="cuda:0") for _ in per]
        d_live = [torch.zeros(1, dtype=torch.int32, device="cuda:0") for _ in per]
        d_plane = device(plane)
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        on_host = None
        for p in per:
            t.rayTrace(frame_dev, W, H, p, kernel=2, sync=False)
            kw = dict(stream=side.cuda_stream, sync=False)
            assert t.tileStopSelect(d_tiles, d_stop[p], 20, W, H, dilate=0, stats=d_stats[p], **kw) is None
            t.momentsAccumulateTiles(d_prev, d_cur, 6.0, d_mom, d_out[p], d_plane, d_len[p], W, H, **kw)
            t.tileStopOrder(None, d_plane, d_ord[p], d_live[p], **kw)
            if p == 1:  # and host buffers on the context's own stream
                h_stop, h_out, h_len = plane.copy(), np.zeros(4 * W * H, F), np.zeros(W * H, F)
                st = t.tileStopSelect(tiles, h_stop, 20, W, H, dilate=0)
                t.momentsAccumulateTiles(prev, cur, 6.0, mom, h_out, plane, h_len, W, H)
                on_host = (st, h_stop, h_out, h_len)
    for p in per:
        w = host(d_stats[p])
        assert dict(tiles=int(w[0]), active=int(w[1]), stopped_now=int(w[2]), frames=int(w[3])) == exp_st
        assert np.array_equal(host(d_stop[p]), exp_stop)
        assert np.array_equal(bits(host(d_out[p])), bits(exp_mom)) and np.array_equal(bits(host(d_len[p])), bits(exp_len))
        assert np.array_equal(host(d_ord[p]), exp_order) and host(d_live[p])[0] == exp_live
    assert on_host[0] == exp_st and np.array_equal(on_host[1], exp_stop)
    assert np.array_equal(bits(on_host[2]), bits(exp_mom)) and np.array_equal(bits(on_host[3]), bits(exp_len))
    assert exp_st["stopped_now"] > 0 and exp_st["active"] > 0


# ---- ProgressiveViewHIP::setAdaptive through rt_render --events ----------------------------------

VW, VH = 64, 48
PX = VW * VH
TILES = ar.n_tiles(VW, VH)
# the configuration of tests/test_adaptive_host.py's precondition: on the CPU, over the oracle's frames of
# this view, 17, 15, 13, 13, 13, 13, 12, 12, 11 tiles of 48 are live after displays 4 to 12
RULE = dict(threshold=0.2, max_ratio=4.0, min_frames=4, dilate=0)
MIN_FRAMES = 4
EVENTS = ",".join(["d"] * 13 + ["l"] + ["d"] * 6)
CONVERGE = ["--converge", "0.001", "--converge-min-frames", str(MIN_FRAMES)]  # (the frame-wide rule never fires here)
ADAPTIVE = ["--adaptive", "0.2", "--adaptive-max-ratio", "4", "--adaptive-min-frames", "4", "--adaptive-dilate", "0"]


def run_cli(tmp, args, outputs, width=VW, height=VH, stop_map=True):
    """vr.run_view with the meter's tile map and the stop planes beside its own files."""
    tiles, stops = tmp / "noise_map.f32", tmp / "stop_map.u32"
    for f in (tiles, stops):
        f.unlink(missing_ok=True)
    extra = ["--noise-map-out", str(tiles)] + (["--stop-map-out", str(stops)] if stop_map else [])
    r = vr.run_view(tmp, args + extra, outputs, width, height)
    r["map"] = np.fromfile(tiles, F)
    r["stops"] = np.fromfile(stops, U) if stop_map else None
    return r


@pytest.fixture(scope="module")
def view_runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("adaptive_view")
    base = ["--mesh", "2000", "--events", EVENTS] + CONVERGE
    return run_cli(tmp, base + ADAPTIVE, ("shown", "raw")), run_cli(tmp, base, ("shown", "raw"), stop_map=False)


def test_view_follows_the_rule(view_runs):
    """Thirteen displays, a key, six more.  Every stop plane is the restatement applied to that display's
    tile map and the plane before it; `tiles_active` is in every line; raw frame k + 1 differs from raw frame
    k only in the live tiles of plane k, and there it is the frame of the same run without --adaptive — in
    every tile that has been traced at every display so far: a tile that was stopped kept its seeds, so after
    the key, live again, it draws other samples than the run that never stopped it; the plane is zero again
    after the key, and the tiles it had stopped are traced again."""
    on, off = view_runs
    lines = on["lines"][:-1]
    assert [l["event"] for l in lines] == EVENTS.split(",") and all("tiles_active" in l for l in lines)
    assert all("tiles_active" not in l for l in off["lines"])
    n_displays = EVENTS.count("d")
    assert on["stops"].size == TILES * n_displays and on["map"].size == 2 * TILES * n_displays
    assert on["raw"].size == off["raw"].size == 4 * PX * n_displays
    assert np.array_equal(bits(on["shown"]), bits(on["raw"]))  # what is displayed is the accumulation buffer
    plane = np.zeros(TILES, U)
    ever = np.zeros(TILES, bool)  # stopped at some display so far: its seeds are no longer the other run's
    pixel_tile = ar.pixel_tiles(VW, VH)
    k, progression, active = 0, -1, []
    for l in lines:
        if l["event"] == "l":
            plane, progression = np.zeros(TILES, U), 0  # every tile is live again; the next display is progression 1
            continue
        progression += 1
        n = max(progression, 1)
        assert l["rendered"] is True and l["progression"] == progression and l["converged"] is False, l
        raw, raw_off = (a[4 * PX * k:4 * PX * (k + 1)] for a in (on["raw"], off["raw"]))
        live = np.repeat(ar.pixel_mask(plane, VW, VH), 4)  # the plane this display was rendered under
        same_seeds = np.repeat(~ever[pixel_tile], 4)
        assert np.array_equal(bits(raw)[same_seeds], bits(raw_off)[same_seeds]), k
        if k:
            last, last_off = (a[4 * PX * (k - 1):4 * PX * k] for a in (on["raw"], off["raw"]))
            assert np.array_equal(bits(raw)[~live], bits(last)[~live]), k
            # a tile that is live again after having been stopped: wherever the other run's frame changed in
            # it, this run's did
            moved = np.flatnonzero(ever & (plane == 0))
            for t in moved:
                px = np.repeat(pixel_tile == t, 4)
                if not np.array_equal(bits(raw_off)[px], bits(last_off)[px]):
                    assert not np.array_equal(bits(raw)[px], bits(last)[px]), (k, t)
            assert (k == 13) == (moved.size > 0) or k > 13
        tiles = on["map"][2 * TILES * k:2 * TILES * (k + 1)]
        if n >= MIN_FRAMES:
            plane, st = ar.select(tiles, plane, n, VW, VH, **RULE)
        assert np.array_equal(on["stops"][TILES * k:TILES * (k + 1)], plane), k
        ever |= plane != 0
        assert l["tiles_active"] == int((plane == 0).sum()), l
        active.append(l["tiles_active"])
        k += 1
    print("live tiles per display:", active)
    first = active[:13]
    assert first[:4] == [TILES] * 4 and len(set(first[4:])) >= 3 and 0 < min(first) and max(first[4:]) < TILES
    assert active[13:16] == [TILES] * 3 and active[16] < TILES  # zero again after the key (n = 1, 2, 3), then the rule again
    assert not np.array_equal(bits(on["raw"]), bits(off["raw"]))  # the stopped tiles did stay behind


def test_flag_absent_changes_nothing(tmp_path, pt, tracer, golden):
    """Two runs without --adaptive, every display stage that keeps moments on: byte-equal, and the frames
    tests/view_ref.py recomposes."""
    flags = vr.Flags(variance_guided=True)
    events = ",".join(["d"] * 6 + ["l"] + ["d"] * 3)
    args = ["--mesh", "2000", "--events", events, "--tonemap"] + flags.cli() + CONVERGE
    a = run_cli(tmp_path, args, ("shown", "raw", "feat", "f8"), stop_map=False)
    b = run_cli(tmp_path, args, ("shown", "raw", "feat", "f8"), stop_map=False)
    for name in ("shown", "raw", "feat", "f8", "map"):
        assert a[name].size and np.array_equal(bits(a[name]), bits(b[name])), name
    assert a["lines"] == b["lines"] and all("tiles_active" not in l for l in a["lines"])
    g = golden(CASE)  # (the CLI's --mesh 2000 is the golden case's mesh; no event moves it)
    exp = vr.displayed(tracer, pt.scenes, flags, events, a["raw"], a["feat"], VW, VH, mesh=(g["verts"], g["idx"]))
    assert np.array_equal(bits(a["shown"]), bits(np.concatenate(exp.frames)))


def test_view_converges_when_no_tile_is_live(tmp_path):
    """A small frame and a threshold nothing exceeds: every tile stops at the first allowed display, the
    view reports converged there, and no later display traces."""
    events = ",".join(["d"] * 6)
    args = ["--mesh", "2000", "--events", events, "--converge", "1e-9", "--converge-min-frames", "2", "--adaptive", "1e30",
            "--adaptive-max-ratio", "inf", "--adaptive-min-frames", "2", "--adaptive-dilate", "1"]
    r = run_cli(tmp_path, args, ("raw",), 16, 16)
    lines = r["lines"][:-1]
    assert [l["rendered"] for l in lines] == [True, True, True, False, False, False]
    assert [l["tiles_active"] for l in lines] == [4, 4, 0, 0, 0, 0]
    assert [l["converged"] for l in lines] == [False, False, True, True, True, True]
    assert [l["redisplay"] for l in lines] == [True, True, False, False, False, False]
    assert r["raw"].size == 3 * 4 * 16 * 16 and np.array_equal(r["stops"][-4:], np.full(4, 2, U))
