"""GPU: the first-hit feature buffers (rt_render_features) against the oracle's
closest hits and float32 numpy restatements, bit for bit; and that neither they nor the denoiser
disturb a render.  Run on the MI355X box with `pytest -m gpu`."""
from __future__ import annotations

import numpy as np
import pytest

import features_ref as fr
from conftest import bits

pytestmark = pytest.mark.gpu

CASE = "tris_64x48_sr1"  # 2,000 triangles, 91 % mesh pixels
SIZES = [(64, 48), (61, 47)]


def _tracer(pt, g, m, builder="host"):
    rt = pt.RayTracer(0)
    rt.setSpheres(g["spheres"].view(pt._abi.SPHERE_DTYPE))
    rt.setCamera(g["camera"])
    rt.setSampleRate(m["sample_rate"])
    rt.setMaxPathDepth(m["max_depth"])
    rt.setNDRange(m["nd_y"])
    rt.setBuilder(builder)
    rt.setMesh(g["verts"], g["idx"])
    rt.setSeeds(m["Wpad"], m["Hpad"], g["seeds_in"])
    return rt


@pytest.fixture(scope="module")
def expected(pt, oracle, golden):
    """Per frame size: the primary rays, the oracle's closest hits and the restated feature buffer."""
    g = golden(CASE)
    lib, ab = pt.load_library(), pt._abi
    out = {}
    for W, H in SIZES:
        cam = np.ascontiguousarray(g["camera"], np.float32)
        rays = np.zeros(W * H, ab.RAY_DTYPE)
        assert lib.rt_primary_rays(ab.ptr(cam), W, H, ab.ptr(rays)) == ab.RT_OK
        ids, t = oracle.closest_hits(rays, np.ascontiguousarray(g["verts"]), np.ascontiguousarray(g["idx"]))
        out[(W, H)] = (rays, ids, t, fr.features_tris(oracle, rays, g["verts"], g["idx"]))
    return out


@pytest.mark.parametrize("builder", ["host", "gpu"])
def test_features_tris(builder, tracer, pt, golden, golden_meta, expected):
    g, m = golden(CASE), golden_meta["cases"][CASE]
    rt = _tracer(pt, g, m, builder)
    for W, H in SIZES:
        rays, ids, t, exp = expected[(W, H)]
        # the context's camera and rays are the host helper's
        assert np.array_equal(rt.primaryRays(W, H).view(np.uint8), rays.view(np.uint8))
        o, d = np.ascontiguousarray(rays["o"]), np.ascontiguousarray(rays["d"])
        first = None
        for trav in ("bvh", "bvh4f", "linear"):
            rt.setTraversal(trav)
            feat = np.full(2 * W * H * 4, np.nan, np.float32)
            rt.renderFeatures(feat, W, H, kernel=pt.RayTracer.KERNEL_TRIS)
            f = feat.reshape(2, W * H, 4)
            fid = fr.feature_ids(feat)
            hit = ids >= 0
            assert 0.85 < hit.mean() < 0.95
            # id and t: the oracle's closest hits (the reference's linear loop)
            assert np.array_equal(fid[hit], ids[hit]), (builder, trav, W, H)
            assert np.array_equal(bits(f[0, hit, 3]), bits(t[hit]))
            # P = o + d * t, N = normalize(cross3(e2, e1)): float32 restatements
            assert np.array_equal(bits(f[0, hit, :3]), bits(fr.hit_points(o[hit], d[hit], t[hit])))
            assert np.array_equal(bits(f[1, hit, :3]), bits(fr.mesh_normals(g["verts"], g["idx"], ids[hit])))
            # box pixels: exactly the oracle's misses (the camera is inside the box)
            assert np.array_equal(fid == fr.RT_FEAT_BOX, ~hit) and not np.any(fid == fr.RT_FEAT_NONE)
            Pb, Nb, tb = f[0, ~hit, :3], f[1, ~hit, :3], f[0, ~hit, 3]
            assert np.array_equal(bits(Pb), bits(fr.hit_points(o[~hit], d[~hit], tb)))
            axis = np.abs(Nb).argmax(axis=1)
            r = np.arange(len(Pb))
            assert np.array_equal(np.abs(Nb).sum(axis=1), np.ones(len(Pb), np.float32))  # a unit axis vector
            half = np.array(fr.BOX, np.float32)[axis]
            # rounding of o + d * t at magnitude <= 12: a few ulp of 8, about 4e-6
            assert np.abs(np.abs(Pb[r, axis]) - half).max() <= 1e-5
            assert np.array_equal(Nb[r, axis], -np.sign(Pb[r, axis]))
            # and the whole buffer equals the restatement (box t and normal included)
            assert np.array_equal(bits(feat), bits(exp.reshape(-1))), (builder, trav, W, H)
            if first is None:
                first = feat
            assert np.array_equal(bits(feat), bits(first))
        rt.setTraversal("bvh")
    # a device tensor receives the same bits, and the time of the kernel is reported
    import torch

    W, H = SIZES[1]
    dev = torch.zeros(2 * W * H * 4, dtype=torch.float32, device="cuda:0")
    rt.renderFeatures(dev, W, H, kernel=2)
    assert np.array_equal(bits(dev.cpu().numpy()), bits(expected[(W, H)][3].reshape(-1)))
    assert rt.lastFeaturesMs() > 0.0
    rt.close()


def test_features_errors(tracer, pt):
    ab = pt._abi
    rt = pt.RayTracer(0)
    feat = np.zeros(2 * 8 * 8 * 4, np.float32)
    with pytest.raises(ab.RtError) as e:
        rt.renderFeatures(feat, 8, 8, kernel=2)
    assert e.value.status == ab.RT_ERR_NO_MESH
    with pytest.raises(ab.RtError) as e:
        rt.renderFeatures(feat, 8, 8, kernel=0)
    assert e.value.status == ab.RT_ERR_NO_SCENE
    with pytest.raises(ValueError):
        rt.renderFeatures(feat[:-1], 8, 8, kernel=2)
    rt.close()


def _info(rt):
    i = rt.renderInfo()
    i.pop("schedule_host_ms")  # a host time, not a state
    return i


def test_features_and_denoise_do_not_disturb_renders(tracer, pt, golden, golden_meta):
    """The golden frames rendered with a features call and a denoise call after every frame (host
    buffers and device tensors, the context's stream and another one) keep the fixture's bits and
    final seeds; counters, render info and rt_read's framebuffer are those of a run without the
    calls."""
    import torch

    g, m = golden(CASE), golden_meta["cases"][CASE]
    W, H = m["W"], m["H"]
    plain = _tracer(pt, g, m)
    exp_state = []
    out = np.zeros(W * H * 4, np.float32)
    for p in range(m["frames"]):
        plain.rayTrace(out, W, H, p, kernel=2)
        exp_state.append((plain.counters(), _info(plain)))
    plain.close()

    rt = _tracer(pt, g, m)
    out = np.zeros(W * H * 4, np.float32)
    feat = np.zeros(2 * W * H * 4, np.float32)
    den = np.zeros(W * H * 4, np.float32)
    dfeat = torch.zeros(2 * W * H * 4, dtype=torch.float32, device="cuda:0")
    dsrc = torch.zeros(W * H * 4, dtype=torch.float32, device="cuda:0")
    side = torch.cuda.Stream()
    back = np.zeros(W * H * 4, np.float32)
    for p in range(m["frames"]):
        rt.rayTrace(out, W, H, p, kernel=2)
        assert np.array_equal(bits(out), bits(g["frames"][p])), f"frame {p}"
        if p % 2 == 0:
            rt.renderFeatures(feat, W, H, kernel=2)
            rt.denoise(out, feat, den, W, H)
        else:
            dsrc.copy_(torch.from_numpy(out))
            torch.cuda.synchronize()
            rt.renderFeatures(dfeat, W, H, kernel=2, stream=side.cuda_stream, sync=False)
            rt.denoise(dsrc, dfeat, dsrc, W, H, stream=side.cuda_stream, sync=False)
        assert rt.counters() == exp_state[p][0]
        assert _info(rt) == exp_state[p][1]
        rt.read(back)
        assert np.array_equal(bits(back), bits(g["frames"][p]))
        assert np.array_equal(bits(out), bits(g["frames"][p]))  # the filter's input is only read
    torch.cuda.synchronize()
    assert np.array_equal(rt.getSeeds(), g["seeds_out"])
    assert rt.lastKernelMs() > 0.0
    rt.close()


@pytest.mark.parametrize("W,H", [(64, 64), (50, 33)])
def test_features_spheres(W, H, tracer, pt):
    """main_scene under MAIN_CAMERA.  Surface ids against a float64 analytic classification on every
    pixel whose float64 answer is stable under a +-1e-5 perturbation of d (cap on the pixels left
    out: 2 % of the frame; computed on the CPU for these two frames: 0 pixels, 0 %, at both sizes:
    52 % / 65 % sphere pixels, the rest box)."""
    sc, ab = pt.scenes, pt._abi
    S = np.asarray(sc.main_scene(), ab.SPHERE_DTYPE).reshape(-1)
    cam = sc.camera_spherical(W, **sc.MAIN_CAMERA)
    rt = pt.RayTracer(0)
    rt.setSpheres(S)
    rt.setCamera(cam)
    rays = rt.primaryRays(W, H)
    o, d = np.ascontiguousarray(rays["o"]), np.ascontiguousarray(rays["d"])
    ids64, stable = fr.stable_spheres64(o, d, S["center"], S["radius"])
    assert (~stable).mean() <= 0.02
    first = None
    for kernel in (pt.RayTracer.KERNEL_SPHERES, pt.RayTracer.KERNEL_SPHERES_SS):
        feat = np.full(2 * W * H * 4, np.nan, np.float32)
        rt.renderFeatures(feat, W, H, kernel=kernel)
        f = feat.reshape(2, W * H, 4)
        fid = fr.feature_ids(feat)
        assert np.array_equal(fid[stable], ids64[stable])
        sph = fid <= fr.RT_FEAT_SPHERE0
        assert 0.4 < sph.mean() < 0.8
        s = fr.RT_FEAT_SPHERE0 - fid[sph]
        c, r = S["center"][s].astype(np.float64), S["radius"][s].astype(np.float64)
        P, N, t = f[0, sph, :3], f[1, sph, :3], f[0, sph, 3]
        assert np.array_equal(bits(P), bits(fr.hit_points(o[sph], d[sph], t)))
        dist = np.sqrt(((P.astype(np.float64) - c) ** 2).sum(axis=1))
        assert np.all(np.abs(dist - r) <= 1e-4 * r)
        assert np.abs(N.astype(np.float64) - (P.astype(np.float64) - c) / r[:, None]).max() <= 1e-5
        # the others: the box, as in the triangle kernel
        box = fid == fr.RT_FEAT_BOX
        assert np.array_equal(box, ~sph)
        bt, ok, Pb, Nb = fr.box_hits(o[box], d[box])
        assert ok.all()
        assert np.array_equal(bits(f[0, box, 3]), bits(bt)) and np.array_equal(bits(f[0, box, :3]), bits(Pb))
        assert np.array_equal(bits(f[1, box, :3]), bits(Nb))
        if first is None:
            first = feat
        assert np.array_equal(bits(feat), bits(first))
    rt.close()
