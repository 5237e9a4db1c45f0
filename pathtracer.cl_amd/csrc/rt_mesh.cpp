/*
 * rt_mesh.cpp — the mesh of a context (librtmi.so host runtime): the build and upload of both
 * trees (rt_set_mesh), the moving mesh (rt_update_mesh: the GPU refit of rt_refit.hip or a
 * rebuild), what a caller can read back of them, and the synthetic test mesh.
 */
#include <cmath>
#include <cstring>
#include <thread>

#include "rt_ctx.h"
#include "rt_math.h"
#include "rt_quant.h"

namespace {

/* The levels of the compressed 4-wide tree rooted at `root` as node index ranges [lo, hi), level 0
   the root (q4: every node's RT_QNODE_DWORDS, n nodes; the links are dwords 12-15).  Both builders
   number a tree breadth-first, so level k + 1 starts where level k ends; the walk checks that on
   the links themselves and returns the levels it could confirm (the shadow cache's cut is one of
   them, or none).  A subtree's levels (adjoining = false: the cone split's subtree A, whose nodes
   precede its sibling's on every level) are index ranges too, each somewhere after the one before. */
std::vector<std::pair<uint32_t, uint32_t>> tree_levels(const uint32_t *q4, uint32_t n, uint32_t root,
                                                       bool adjoining = true)
{
    std::vector<std::pair<uint32_t, uint32_t>> lv;
    if (!q4 || root >= n) return lv;
    uint32_t lo = root, hi = root + 1u;
    for (;;) {
        lv.emplace_back(lo, hi);
        uint32_t cmin = ~0u, cmax = 0u, cnt = 0u;
        for (uint32_t i = lo; i < hi; ++i)
            for (int k = 0; k < 4; ++k) {
                const int32_t code = (int32_t)q4[(size_t)i * RT_QNODE_DWORDS + 12 + k];
                if (code < 0 || code == RT_EMPTY_CHILD) continue;
                cmin = std::min(cmin, (uint32_t)code);
                cmax = std::max(cmax, (uint32_t)code);
                ++cnt;
            }
        if (!cnt) break;
        if ((adjoining ? cmin != hi : cmin < hi) || cmax - cmin + 1u != cnt || cmax >= n) break; /* not a contiguous next level */
        lo = cmin;
        hi = cmax + 1u;
    }
    return lv;
}

} // namespace

extern "C" {

/* The mesh's bounds, padded: the box of the vertices the triangles use, grown by 1e-3 of its
   extent + 1e-4 — every point of every triangle (and every point the kernel's triangle test can
   accept: its error is orders of magnitude below the pad) lies at least the pad inside, so a ray
   segment that misses the padded box meets no triangle (k_tris answers such box-path queries
   without a traversal). False when the vertices are not finite (validation reports it). */
static bool mesh_bounds(const float *verts, const int32_t *idx, uint32_t n_tris, float lo[3], float hi[3])
{
    for (int k = 0; k < 3; ++k) {
        lo[k] = INFINITY;
        hi[k] = -INFINITY;
    }
    for (uint64_t i = 0; i < 3ull * n_tris; ++i) {
        const float *v = verts + 3ull * (uint32_t)idx[i];
        for (int k = 0; k < 3; ++k) {
            lo[k] = std::min(lo[k], v[k]);
            hi[k] = std::max(hi[k], v[k]);
        }
    }
    float ext = 0.0f;
    for (int k = 0; k < 3; ++k) {
        if (!std::isfinite(lo[k]) || !std::isfinite(hi[k])) return false;
        ext = std::max(ext, hi[k] - lo[k]);
    }
    const float pad = 1e-3f * ext + 1e-4f;
    for (int k = 0; k < 3; ++k) {
        lo[k] -= pad;
        hi[k] += pad;
    }
    return true;
}

/* The old mesh's trees and records go before the new ones are made. */
static void drop_mesh(rt_ctx *c)
{
    c->d_nodes4.reset();
    c->d_nodes4q.reset();
    c->d_tris.reset();
    c->n_tris = 0;
}

/* set_mesh_build with a GPU builder (rt_build_gpu.hip; `kind`: RT_BUILD_GPU or
   RT_BUILD_GPU_PLOC): one tree over every triangle for every query, its arrays made on the
   device and taken over here.  With RT_BUILD_OPT_LIGHTS (`opts`) the device build does what the
   host build below does around its trees, under the same knobs: the never_hit triangles left out
   (RT_CULL_UNHITTABLE, not in dynamic mode), and a shadow tree after the first whose root keeps
   the lights' possible occluders (A) and the rest (B) apart (RT_LIGHT_CONE), in the host
   build's layout; without a split, one tree. */
static int set_mesh_build_gpu(rt_ctx *c, const float *verts, uint32_t n_verts, const int32_t *idx, uint32_t n_tris,
                              int kind, bool dynamic, uint32_t opts, int collapse)
{
    std::string err;
    if (!rt_validate_mesh(verts, n_verts, idx, n_tris, err)) return fail(c, RT_ERR_ARG, err);
    drop_mesh(c);
    RtGpuBvh g;
    bool det_cull = true;
    if (const char *v = getenv("RT_DET_CULL")) det_cull = atoi(v) != 0; /* A/B knob */
    RtGpuBuildLights bl;
    std::vector<float> lights;
    if (opts & RT_BUILD_OPT_LIGHTS) {
        bl.cull = true;
        if (const char *v = getenv("RT_CULL_UNHITTABLE")) bl.cull = atoi(v) != 0; /* A/B knob */
        if (dynamic) bl.cull = false; /* rt_set_mesh_dynamic: every later update can refit */
        bool cone = kLightCone;
        if (const char *v = getenv("RT_LIGHT_CONE")) cone = atoi(v) != 0; /* A/B knob */
        if (cone && bl.cull)
            for (const rt_sphere &L : c->lights) {
                const float w[4] = {L.center.x, L.center.y, L.center.z, L.radius};
                lights.insert(lights.end(), w, w + 4);
            }
        bl.lights = lights.data();
        bl.n_lights = (uint32_t)(lights.size() / 4);
    }
    const int e = rt_build_bvh_gpu(verts, n_verts, idx, n_tris, g, err, c->stream, det_cull, kind == RT_BUILD_GPU_PLOC,
                                   bl.cull ? &bl : nullptr, collapse == RT_COLLAPSE_SAH);
    const bool two = !e && g.n_nodes4_shadow > 0 && g.nodes4q;
    const uint32_t n_all = g.n_nodes4 + (two ? g.n_nodes4_shadow : 0u);
    c->d_nodes4.adopt(g.nodes4, 32ull * g.n_nodes4);
    c->d_nodes4q.adopt(g.nodes4q, (size_t)RT_QNODE_DWORDS * n_all);
    c->d_tris.adopt(g.tris, 12ull * n_tris * (two ? 2u : 1u));
    if (e) return fail(c, RT_ERR_HIP, "GPU BVH build: " + err);
    c->n_tris = n_tris;
    c->mesh_serial++;
    c->bvh.n_nodes = 0; /* no binary layout */
    c->bvh.n_leaves = 0;
    c->bvh.depth = 0;
    c->bvh.n_nodes4 = g.n_nodes4;
    c->bvh.depth4 = g.depth4;
    c->bvh.stack4 = g.stack4;
    c->bvh.build_seconds = g.build_seconds;
    c->bvh.n_hit = bl.cull ? g.n_hit : n_tris; /* (without the option the GPU build keeps every triangle) */
    c->tree_recs = (size_t)n_tris * (two ? 2u : 1u);
    c->shadow_root = two ? g.n_nodes4 : 0u;
    c->n_nodes4_shadow = two ? g.n_nodes4_shadow : 0u;
    c->stack4_all = two ? g.stack4_all : g.stack4;
    c->cone_root = two ? g.n_nodes4 + 1u : 0u; /* A: the shadow root's first child */
    c->n_cone = two ? g.n_cone : 0u;
    c->cone_levels.clear();
    c->cone_lights.clear();
    c->cone_stale = false;
    c->shadow_levels.clear();
    if ((two || c->shadow_cache) && g.nodes4q) { /* the levels of the shadow queries' tree, read from its links */
        std::vector<uint32_t> hq((size_t)RT_QNODE_DWORDS * n_all);
        HIPCHK(c, hipMemcpy(hq.data(), g.nodes4q, hq.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        c->shadow_levels = tree_levels(hq.data(), n_all, c->shadow_root);
        if (two) {
            c->cone_levels = tree_levels(hq.data(), n_all, c->cone_root, false);
            for (float w : lights) {
                uint32_t bits;
                memcpy(&bits, &w, sizeof(bits));
                c->cone_lights.push_back(bits);
            }
        }
    }
    c->mesh_builder = kind;
    c->mesh_build_opts = opts;
    c->mesh_collapse = collapse;
    c->mesh_bounds_ok = mesh_bounds(verts, idx, n_tris, c->mesh_lo, c->mesh_hi);
    c->mesh_det_cull = det_cull;
    c->mesh_dynamic = dynamic;
    return RT_OK;
}

/* The build and the upload of rt_set_mesh (and of rt_update_mesh's rebuild): `builder`, `dynamic`
   `opts` and `collapse` (RT_BUILD_OPT_*, RT_COLLAPSE_*: the device builders') are the context's
   choices for the next mesh, or the current mesh's own. */
static int set_mesh_build(rt_ctx *c, const float *verts, uint32_t n_verts, const int32_t *idx, uint32_t n_tris,
                          int builder, bool dynamic, uint32_t opts, int collapse)
{
    std::string err;
    c->mesh_bounds_ok = false;
    if (builder == RT_BUILD_GPU || builder == RT_BUILD_GPU_PLOC)
        return set_mesh_build_gpu(c, verts, n_verts, idx, n_tris, builder, dynamic, opts, collapse);
    /* Two host trees over the same triangles: the closest-hit queries (camera rays, bounces, the
       seed passes) walk one split by surface area, the shadow queries one whose cost area leans
       toward the scene's lights (rt_bvh.cpp Builder::area) — three quarters of the dragon frame's
       steps are shadow rays from mesh hits, and the lights' tree cuts them 10 %, while the long
       chains' subtree-parallel seed pass (closest hits of box paths over a cut of the tree's top
       levels) ran 1.3 ms slower on it (profiles/r06za).  Built side by side on two host threads;
       the shadow tree's nodes and triangle records follow the first tree's in d_nodes4q / d_tris
       (links offset), so a shadow query only starts at another root.  Culling only: any tree gives
       the same hits. */
    RtBvh b;
    if (const char *v = getenv("RT_CULL_UNHITTABLE")) b.cull_unhittable = atoi(v) != 0; /* A/B knob */
    if (dynamic) b.cull_unhittable = false; /* rt_set_mesh_dynamic: every later update can refit */
    if (const char *v = getenv("RT_DET_CULL")) b.det_cull = atoi(v) != 0; /* A/B knob */
    RtBvh sb;
    sb.cull_unhittable = b.cull_unhittable;
    sb.det_cull = b.det_cull;
    for (const rt_sphere &L : c->lights) {
        sb.light_centres.push_back(L.center.x);
        sb.light_centres.push_back(L.center.y);
        sb.light_centres.push_back(L.center.z);
    }
    if (const char *v = getenv("RT_BVH_LIGHT_W")) sb.light_cost_weight = (float)atof(v); /* A/B knob (0: one tree) */
    /* the lights' cone split of the shadow tree (rt_bvh.cpp never_occludes); RT_LIGHT_CONE=0: the
       build without it */
    bool cone = kLightCone;
    if (const char *v = getenv("RT_LIGHT_CONE")) cone = atoi(v) != 0; /* A/B knob */
    if (cone)
        for (const rt_sphere &L : c->lights) sb.light_radii.push_back(L.radius);
    b.light_cost_weight = 0.0f;
    bool two = !sb.light_centres.empty() && sb.light_cost_weight > 0.0f && 2ull * n_tris < (1ull << 28);
    bool ok2 = false;
    std::string err2;
    std::thread th;
    if (two)
        th = std::thread([&]() {
            try {
                ok2 = rt_build_bvh(verts, n_verts, idx, n_tris, sb, err2);
            } catch (...) {
                ok2 = false;
            }
        });
    bool ok = false;
    try {
        ok = rt_build_bvh(verts, n_verts, idx, n_tris, b, err);
    } catch (...) {
        if (th.joinable()) th.join();
        throw;
    }
    if (th.joinable()) th.join();
    if (!ok)
        return fail(c, err.find("deeper") != std::string::npos ? RT_ERR_LIMIT : RT_ERR_ARG, err);
    two = two && ok2 && !b.nodes4q.empty() && !sb.nodes4q.empty();
    std::vector<uint32_t> q4 = std::move(b.nodes4q);
    std::vector<float> tr = std::move(b.tris);
    const uint32_t n_a = b.n_nodes4;
    if (two) {
        q4.insert(q4.end(), sb.nodes4q.begin(), sb.nodes4q.end());
        for (size_t i = n_a; i < (size_t)n_a + sb.n_nodes4; ++i)
            for (int k = 0; k < 4; ++k) {
                uint32_t &w = q4[i * RT_QNODE_DWORDS + 12 + k]; /* the explicit child links (rt_quant.h) */
                int32_t code = (int32_t)w;
                if (code == RT_EMPTY_CHILD) continue;
                if (code >= 0) {
                    code += (int32_t)n_a;
                } else {
                    const uint32_t enc = (uint32_t)(~code);
                    code = ~(int32_t)((((enc >> 3) + n_tris) << 3) | (enc & 7u));
                }
                w = (uint32_t)code;
            }
        tr.insert(tr.end(), sb.tris.begin(), sb.tris.end());
    }
    c->mesh_builder = RT_BUILD_HOST;
    c->mesh_build_opts = 0; /* (the host build does all of it anyway) */
    c->mesh_collapse = RT_COLLAPSE_SAH; /* (rt_bvh.cpp collapses by the same rule) */
    drop_mesh(c);
    HIPCHK(c, c->d_nodes4.reserve(b.nodes4.size()));
    if (!q4.empty()) HIPCHK(c, c->d_nodes4q.reserve(q4.size()));
    HIPCHK(c, c->d_tris.reserve(tr.size()));
    HIPCHK(c, hipMemcpy(c->d_nodes4, b.nodes4.data(), b.nodes4.size() * sizeof(float), hipMemcpyHostToDevice));
    if (!q4.empty())
        HIPCHK(c, hipMemcpy(c->d_nodes4q, q4.data(), q4.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->d_tris, tr.data(), tr.size() * sizeof(float), hipMemcpyHostToDevice));
    c->tree_recs = tr.size() / 12;
    c->shadow_root = two ? n_a : 0u;
    c->n_nodes4_shadow = two ? sb.n_nodes4 : 0u;
    c->shadow_levels = tree_levels(q4.data(), (uint32_t)(q4.size() / RT_QNODE_DWORDS), c->shadow_root);
    c->cone_root = two && sb.cone_root4 ? n_a + sb.cone_root4 : 0u;
    c->n_cone = c->cone_root ? sb.n_cone : 0u;
    c->cone_levels.clear();
    c->cone_lights.clear();
    c->cone_stale = false;
    if (c->cone_root) {
        c->cone_levels = tree_levels(q4.data(), (uint32_t)(q4.size() / RT_QNODE_DWORDS), c->cone_root, false);
        for (const rt_sphere &L : c->lights) {
            const float w[4] = {L.center.x, L.center.y, L.center.z, L.radius};
            uint32_t bits[4];
            memcpy(bits, w, sizeof(bits));
            c->cone_lights.insert(c->cone_lights.end(), bits, bits + 4);
        }
    }
    c->stack4_all = two ? std::max(b.stack4, sb.stack4) : b.stack4;
    c->n_tris = n_tris;
    c->mesh_serial++;
    c->bvh.n_nodes = b.n_nodes;
    c->bvh.n_leaves = b.n_leaves;
    c->bvh.depth = b.depth;
    c->bvh.n_nodes4 = b.n_nodes4;
    c->bvh.depth4 = b.depth4;
    c->bvh.stack4 = b.stack4;
    c->bvh.build_seconds = b.build_seconds;
    c->bvh.n_hit = b.n_hit;
    c->mesh_bounds_ok = mesh_bounds(verts, idx, n_tris, c->mesh_lo, c->mesh_hi);
    c->mesh_det_cull = b.det_cull;
    c->mesh_dynamic = dynamic;
    return RT_OK;
}

/* The refit's workspace for the current mesh: the levels of both trees read off their links
   (deepest first: the steps of k_refit_levels), and every array an update writes.  Nothing is
   allocated in an update after this. */
static int refit_prepare(rt_ctx *c)
{
    rt_ctx::Refit &r = c->refit;
    const uint32_t n_a = c->bvh.n_nodes4, n_s = c->n_nodes4_shadow, n_all = n_a + n_s;
    std::vector<uint32_t> q((size_t)RT_QNODE_DWORDS * n_all, 0u);
    if (c->d_nodes4q) {
        HIPCHK(c, hipMemcpy(q.data(), c->d_nodes4q, q.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    } else { /* full-precision nodes only: their links in the compressed nodes' place */
        std::vector<float> f(32ull * n_a);
        HIPCHK(c, hipMemcpy(f.data(), c->d_nodes4, f.size() * sizeof(float), hipMemcpyDeviceToHost));
        for (uint32_t i = 0; i < n_a; ++i) memcpy(&q[(size_t)i * RT_QNODE_DWORDS + 12], &f[32ull * i + 24], 16);
    }
    const auto la = tree_levels(q.data(), n_all, 0u);
    const auto ls = n_s ? tree_levels(q.data(), n_all, c->shadow_root) : std::vector<std::pair<uint32_t, uint32_t>>();
    uint64_t seen_a = 0, seen_s = 0;
    for (const auto &l : la) seen_a += l.second - l.first;
    for (const auto &l : ls) seen_s += l.second - l.first;
    if (seen_a != n_a || seen_s != n_s || (!la.empty() && la.back().second != n_a) ||
        (!ls.empty() && (ls.front().first != n_a || ls.back().second != n_all)))
        return fail(c, RT_ERR_STATE, "the tree's levels are not index ranges: no refit");
    r.steps.clear();
    for (size_t d = std::max(la.size(), ls.size()); d-- > 0;) {
        RtRefitStep s = {0u, 0u, 0u, 0u};
        if (d < la.size()) s.a_first = la[d].first, s.a_count = la[d].second - la[d].first;
        if (d < ls.size()) s.s_first = ls[d].first, s.s_count = ls[d].second - ls[d].first;
        r.steps.push_back(s);
    }
    HIPCHK(c, r.d_steps.reserve(r.steps.size()));
    HIPCHK(c, hipMemcpy(r.d_steps, r.steps.data(), r.steps.size() * sizeof(RtRefitStep), hipMemcpyHostToDevice));
    HIPCHK(c, r.d_verts.reserve(3ull * c->n_verts));
    HIPCHK(c, r.d_tbox.reserve(6ull * c->tree_recs));
    HIPCHK(c, r.d_hit0.reserve(c->bvh.n_hit));
    if (n_s) HIPCHK(c, r.d_shadow_full.reserve(32ull * n_s));
    if (!c->d_nodes4q) HIPCHK(c, r.d_qscratch.reserve((size_t)RT_QNODE_DWORDS * n_all));
    HIPCHK(c, r.d_nbox.reserve(rt_refit_nbox_bytes() * n_all));
    HIPCHK(c, r.d_res.reserve(RT_REFIT_RES_WORDS));
    HIPCHK(c, r.d_part.reserve(RT_REFIT_AREA_BLOCKS));
    if (c->cone_root && c->mesh_builder != RT_BUILD_HOST && !c->cone_lights.empty()) { /* k_refit_cone's lights */
        HIPCHK(c, r.d_cone_lights.reserve(c->cone_lights.size()));
        HIPCHK(c, hipMemcpy(r.d_cone_lights, c->cone_lights.data(), c->cone_lights.size() * sizeof(uint32_t),
                            hipMemcpyHostToDevice));
    }
    HIPCHK(c, r.ev0.create());
    HIPCHK(c, r.ev1.create());
    r.ready = true;
    return RT_OK;
}

/* rt_set_mesh, and rt_update_mesh's rebuild: the build, then what a later update needs of this
   mesh — its indices on the host and on the device. */
static int set_mesh_keep(rt_ctx *c, const float *verts, uint32_t n_verts, const int32_t *idx, uint32_t n_tris,
                         int builder, bool dynamic, uint32_t opts, int collapse)
{
    c->refit = rt_ctx::Refit(); /* the refit's workspace: gone with the mesh it was sized for */
    c->have_update = false;
    const int st = set_mesh_build(c, verts, n_verts, idx, n_tris, builder, dynamic, opts, collapse);
    if (st != RT_OK) return st;
    if (idx != c->h_idx.data()) c->h_idx.assign(idx, idx + 3ull * n_tris);
    c->n_verts = n_verts;
    c->d_idx.reset();
    HIPCHK(c, c->d_idx.reserve(3ull * n_tris));
    HIPCHK(c, hipMemcpy(c->d_idx, idx, 12ull * n_tris, hipMemcpyHostToDevice));
    c->d_pose.reset(); /* the pose the trees now hold (rt_mesh_pose) */
    HIPCHK(c, c->d_pose.reserve(3ull * n_verts));
    HIPCHK(c, hipMemcpy(c->d_pose, verts, 12ull * n_verts, hipMemcpyHostToDevice));
    return dynamic ? refit_prepare(c) : RT_OK;
}

int rt_set_mesh(rt_ctx *c, const float *verts, uint32_t n_verts, const int32_t *idx, uint32_t n_tris)
try {
    if (!c || !verts || !idx || !n_verts || !n_tris) return fail(c, RT_ERR_ARG, "empty mesh");
    HIPCHK(c, hipSetDevice(c->device));
    return set_mesh_keep(c, verts, n_verts, idx, n_tris, c->builder, c->dynamic, c->build_opts, c->collapse);
} RT_CATCH(err_of(c))

int rt_set_mesh_dynamic(rt_ctx *c, int on)
try {
    if (!c) return RT_ERR_ARG;
    c->dynamic = on != 0;
    return RT_OK;
} RT_CATCH(err_of(c))

int rt_last_mesh_update(const rt_ctx *c, rt_mesh_update_info *out)
try {
    if (!c || !out) return RT_ERR_ARG;
    if (!c->n_tris) return RT_ERR_NO_MESH;
    if (!c->have_update) return RT_ERR_STATE;
    *out = c->last_update;
    return RT_OK;
} RT_CATCH(err_of(c))

/* rt_update_mesh's other way: the mesh built again from the kept indices, as it was built */
static int update_rebuild(rt_ctx *c, const float *verts, int flags, uint32_t reason, uint32_t newly)
{
    std::vector<float> hv;
    if (flags & RT_MESH_VERTS_DEVICE) {
        hv.resize(3ull * c->n_verts);
        HIPCHK(c, hipMemcpy(hv.data(), c->refit.d_verts, hv.size() * sizeof(float), hipMemcpyDeviceToHost));
        verts = hv.data();
    }
    const std::vector<int32_t> idx = std::move(c->h_idx);
    c->h_idx.clear();
    const int st = set_mesh_keep(c, verts, c->n_verts, idx.data(), c->n_tris, c->mesh_builder, c->mesh_dynamic,
                                 c->mesh_build_opts, c->mesh_collapse);
    if (st != RT_OK) return st;
    c->last_update = {RT_MESH_UPDATE_REBUILT, reason, newly, 0u, 1.0f, 0.0f};
    c->have_update = true;
    return RT_OK;
}

int rt_update_mesh(rt_ctx *c, const float *verts, uint32_t n_verts, int flags)
try {
    if (!c || !verts) return fail(c, RT_ERR_ARG, "rt_update_mesh: null argument");
    if (!c->n_tris || !c->d_nodes4 || !c->d_tris || !c->d_idx) return fail(c, RT_ERR_NO_MESH, "no mesh to update");
    if (n_verts != c->n_verts) return fail(c, RT_ERR_ARG, "rt_update_mesh: the vertex count differs from the mesh's");
    HIPCHK(c, hipSetDevice(c->device));
    rt_ctx::Refit &r = c->refit;
    if (!r.ready) {
        const int st = refit_prepare(c);
        if (st != RT_OK) {
            c->refit = rt_ctx::Refit();
            return st;
        }
    }
    hipStream_t st = c->stream;
    const uint32_t n_tris = c->n_tris, n_hit = c->bvh.n_hit, n_a = c->bvh.n_nodes4;
    uint32_t res[RT_REFIT_RES_WORDS] = {0u, 0u, 0u, 0u, ~0u, ~0u, ~0u, 0u, 0u, 0u, 0u};
    HIPCHK(c, hipMemcpyAsync(r.d_verts, verts, 12ull * n_verts,
                             (flags & RT_MESH_VERTS_DEVICE) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(r.d_res, res, sizeof(res), hipMemcpyHostToDevice, st));
    /* look first: nothing of the mesh is written before the host has decided */
    if (int e = rt_launch_refit_check(r.d_verts, n_verts, c->d_idx, n_tris, c->d_tris, n_hit, r.d_res, st))
        return hip_fail(c, (hipError_t)e, "k_refit_check");
    HIPCHK(c, hipMemcpyAsync(res, r.d_res, sizeof(res), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    if (res[RT_REFIT_RES_BAD] & 1u) return fail(c, RT_ERR_ARG, "non-finite or out-of-range vertex coordinate");
    if (res[RT_REFIT_RES_BAD]) return fail(c, RT_ERR_STATE, "rt_update_mesh: a record's triangle index is out of range");
    if (res[RT_REFIT_RES_NEWLY])
        return update_rebuild(c, verts, flags, RT_REFIT_NEWLY_HITTABLE, res[RT_REFIT_RES_NEWLY]);
    double part[RT_REFIT_AREA_BLOCKS];
    if (!r.have_area0) { /* the build's own sum, before the first overwrite */
        if (int e = rt_launch_refit_area(c->d_nodes4, n_a, r.d_part, st))
            return hip_fail(c, (hipError_t)e, "k_refit_area");
        HIPCHK(c, hipMemcpyAsync(part, r.d_part, sizeof(part), hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        r.area0 = 0.0;
        for (double p : part) r.area0 += p;
        r.have_area0 = true;
    }
    RtRefitLaunch a;
    a.nodes4 = c->d_nodes4;
    a.nodes4_shadow = r.d_shadow_full;
    a.nodes4q = c->d_nodes4q ? c->d_nodes4q : r.d_qscratch;
    a.nbox = r.d_nbox;
    a.tris = c->d_tris;
    a.tbox = r.d_tbox;
    a.n_nodes4 = n_a;
    a.n_nodes4_shadow = c->n_nodes4_shadow;
    a.n_recs = (uint32_t)c->tree_recs;
    a.det_cull = c->mesh_det_cull;
    a.res = r.d_res;
    HIPCHK(c, hipEventRecord(r.ev0, st));
    if (int e = rt_launch_refit_records(r.d_verts, c->d_idx, n_tris, n_hit, a.n_recs, c->d_tris, r.d_tbox, r.d_hit0,
                                        !r.have_hit0, r.d_res, st))
        return hip_fail(c, (hipError_t)e, "k_refit_records");
    r.have_hit0 = true;
    if (int e = rt_launch_refit_levels(a, r.d_steps, r.steps.data(), (uint32_t)r.steps.size(), st))
        return hip_fail(c, (hipError_t)e, "k_refit_levels");
    double now = 0.0;
    if (int e = rt_launch_refit_area(c->d_nodes4, n_a, r.d_part, st))
        return hip_fail(c, (hipError_t)e, "k_refit_area");
    /* a device build's cone split (RT_BUILD_OPT_LIGHTS): does every parked triangle (B's records,
       slots [n_cone, n_hit) of the shadow tree's half) still never occlude the lights it was made for? */
    const bool recheck_cone = c->cone_root && r.d_cone_lights && c->n_cone < n_hit; /* (the rule reads this pose alone) */
    if (recheck_cone)
        if (int e = rt_launch_refit_cone(c->d_tris, n_tris + c->n_cone, n_hit - c->n_cone, r.d_cone_lights,
                                         (uint32_t)(c->cone_lights.size() / 4), r.d_res, st))
            return hip_fail(c, (hipError_t)e, "k_refit_cone");
    HIPCHK(c, hipEventRecord(r.ev1, st));
    HIPCHK(c, hipMemcpyAsync(res, r.d_res, sizeof(res), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(part, r.d_part, sizeof(part), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    c->mesh_serial++; /* the records have changed: the schedule, the lists and the pilot are the old mesh's */
    /* and the cone split was made for the old ones: the whole shadow tree from here on, unless the
       check above found that it still holds (A's triangles that stopped occluding cost time only) */
    c->cone_stale = !(recheck_cone && res[RT_REFIT_RES_CONE] == 0u);
    if (res[RT_REFIT_RES_BAD]) return fail(c, RT_ERR_STATE, "rt_update_mesh: a link of the tree is out of range");
    /* the compressed form holds every node, or none: a change either way is a rebuild (the
       half-written nodes are replaced with everything else) */
    const bool had_q = c->d_nodes4q != nullptr;
    if (had_q ? res[RT_REFIT_RES_QFAIL] != 0u : res[RT_REFIT_RES_QFAIL] == 0u)
        return update_rebuild(c, verts, flags, RT_REFIT_ENCODING, 0u);
    for (double p : part) now += p;
    /* the off-mesh bounds by mesh_bounds' rule */
    float ext = 0.0f;
    for (int k = 0; k < 3; ++k) {
        auto unkey = [](uint32_t key) { return (key & 0x80000000u) ? (key & 0x7FFFFFFFu) : ~key; }; /* k_prep's f2key */
        const uint32_t ul = unkey(res[RT_REFIT_RES_LO + k]), uh = unkey(res[RT_REFIT_RES_HI + k]);
        memcpy(&c->mesh_lo[k], &ul, 4);
        memcpy(&c->mesh_hi[k], &uh, 4);
        ext = std::max(ext, c->mesh_hi[k] - c->mesh_lo[k]);
    }
    const float pad = 1e-3f * ext + 1e-4f;
    for (int k = 0; k < 3; ++k) {
        c->mesh_lo[k] -= pad;
        c->mesh_hi[k] += pad;
    }
    c->mesh_bounds_ok = true;
    /* the update stands: its vertices are the mesh's pose (after a display-side call that still reads the old one) */
    if (const int w = wait_aux(c, st)) return w;
    HIPCHK(c, hipMemcpyAsync(c->d_pose, r.d_verts, 12ull * n_verts, hipMemcpyDeviceToDevice, st));
    HIPCHK(c, hipStreamSynchronize(st));
    float ms = 0.0f;
    HIPCHK(c, hipEventElapsedTime(&ms, r.ev0, r.ev1));
    c->last_update = {RT_MESH_UPDATE_REFIT, RT_REFIT_OK, 0u, res[RT_REFIT_RES_UNHIT],
                      r.area0 > 0.0 ? (float)(now / r.area0) : 1.0f, ms};
    c->have_update = true;
    return RT_OK;
} RT_CATCH(err_of(c))

int rt_mesh_pose(rt_ctx *c, float *out, uint32_t n_verts, int flags)
try {
    if (!c) return RT_ERR_ARG;
    if (!c->n_tris || !c->d_pose) return fail(c, RT_ERR_NO_MESH, "no mesh set");
    if (!out) return fail(c, RT_ERR_ARG, "rt_mesh_pose: null argument");
    if (n_verts != c->n_verts) return fail(c, RT_ERR_ARG, "rt_mesh_pose: the vertex count differs from the mesh's");
    if (flags & ~RT_OUT_DEVICE) return fail(c, RT_ERR_ARG, "rt_mesh_pose: flags other than RT_OUT_DEVICE");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpy(out, c->d_pose, 12ull * n_verts,
                        (flags & RT_OUT_DEVICE) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost));
    HIPCHK(c, hipStreamSynchronize(nullptr)); /* (a device-to-device copy may return before it is done) */
    return RT_OK;
} RT_CATCH(err_of(c))

int rt_mesh_info(const rt_ctx *c, rt_mesh_stats *out)
try {
    if (!c || !out) return RT_ERR_ARG;
    if (!c->n_tris) return RT_ERR_NO_MESH;
    out->n_tris = c->n_tris;
    out->n_nodes2 = c->bvh.n_nodes;
    out->depth2 = c->bvh.depth;
    out->n_nodes4_shadow = c->n_nodes4_shadow;
    out->n_nodes4 = c->bvh.n_nodes4;
    out->depth4 = c->bvh.depth4;
    out->stack4 = c->bvh.stack4;
    out->builder = (uint32_t)c->mesh_builder;
    out->build_seconds = c->bvh.build_seconds;
    out->n_tris_tree = c->bvh.n_hit;
    out->cone_root = c->cone_root;
    out->n_tris_cone = c->n_cone;
    out->collapse = (uint32_t)c->mesh_collapse;
    return RT_OK;
} RT_CATCH(err_of(c))

int rt_mesh_tree(rt_ctx *c, rt_tree_layout *layout, float *nodes4, uint32_t *nodes4q, float *tris)
try {
    if (!c || !layout) return RT_ERR_ARG;
    if (!c->n_tris || !c->d_nodes4 || !c->d_tris) return RT_ERR_NO_MESH;
    layout->n_nodes4 = c->bvh.n_nodes4;
    layout->n_nodes4_shadow = c->n_nodes4_shadow;
    layout->shadow_root = c->shadow_root;
    layout->n_records = (uint32_t)c->tree_recs;
    layout->compressed = c->d_nodes4q ? 1u : 0u;
    if (nodes4q && !c->d_nodes4q) return fail(c, RT_ERR_STATE, "the mesh has no compressed nodes");
    if (!nodes4 && !nodes4q && !tris) return RT_OK;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (nodes4)
        HIPCHK(c, hipMemcpy(nodes4, c->d_nodes4, (size_t)c->bvh.n_nodes4 * 32 * sizeof(float), hipMemcpyDeviceToHost));
    if (nodes4q)
        HIPCHK(c, hipMemcpy(nodes4q, c->d_nodes4q,
                            ((size_t)c->bvh.n_nodes4 + c->n_nodes4_shadow) * RT_QNODE_DWORDS * sizeof(uint32_t),
                            hipMemcpyDeviceToHost));
    if (tris) HIPCHK(c, hipMemcpy(tris, c->d_tris, c->tree_recs * 12 * sizeof(float), hipMemcpyDeviceToHost));
    return RT_OK;
} RT_CATCH(err_of(c))

/* ---- synthetic meshes ---------------------------------------------------- */

static void mesh_grid(uint32_t n_tris, uint32_t *nt, uint32_t *np)
{
    uint32_t t = 2;
    while (4ull * t * (t - 1) < n_tris) ++t;
    *nt = t;     /* latitude bands */
    *np = 2 * t; /* longitude segments */
}

uint32_t rt_mesh_vertex_count(uint32_t n_tris)
{
    uint32_t nt, np;
    mesh_grid(n_tris, &nt, &np);
    return 2 + (nt - 1) * np;
}

int rt_make_mesh(uint32_t n_tris, float cx, float cy, float cz, float r, float *verts, int32_t *idx)
try {
    if (!n_tris || !verts || !idx) return RT_ERR_ARG;
    uint32_t nt, np;
    mesh_grid(n_tris, &nt, &np);
    const float pi = RT_M_PI_F;
    auto put = [&](uint32_t v, float th, float ph) {
        /* displaced sphere: two bump frequencies, deterministic (rt_math.h only) */
        const float bump = 0.08f * rt_sinf(9.0f * th) * rt_sinf(8.0f * ph) +
                           0.04f * rt_sinf(23.0f * th + 3.0f * ph) * rt_cosf(19.0f * ph - 2.0f * th);
        const float rr = r * (1.0f + bump);
        const float st = rt_sinf(th), ct = rt_cosf(th);
        verts[3ull * v + 0] = cx + rr * st * rt_cosf(ph);
        verts[3ull * v + 1] = cy + rr * ct;
        verts[3ull * v + 2] = cz + rr * st * rt_sinf(ph);
    };
    const uint32_t top = 0, bottom = 1 + (nt - 1) * np;
    put(top, 0.0f, 0.0f);
    put(bottom, pi, 0.0f);
    for (uint32_t i = 1; i < nt; ++i) {
        const float th = pi * (float)i / (float)nt;
        for (uint32_t j = 0; j < np; ++j) put(1 + (i - 1) * np + j, th, 2.0f * pi * (float)j / (float)np);
    }
    auto ring = [&](uint32_t i, uint32_t j) -> int32_t { return (int32_t)(1 + (i - 1) * np + (j % np)); };
    /* winding chosen so that cross(e2, e1) (the reference's normal,
       rtcommon.h:389) points outward */
    uint64_t k = 0;
    auto tri = [&](int32_t a, int32_t b, int32_t c) {
        if (k >= n_tris) return;
        idx[3 * k + 0] = a;
        idx[3 * k + 1] = b;
        idx[3 * k + 2] = c;
        ++k;
    };
    for (uint32_t j = 0; j < np; ++j) tri((int32_t)top, ring(1, j), ring(1, j + 1));
    for (uint32_t i = 1; i + 1 < nt; ++i)
        for (uint32_t j = 0; j < np; ++j) {
            tri(ring(i, j), ring(i + 1, j), ring(i + 1, j + 1));
            tri(ring(i, j), ring(i + 1, j + 1), ring(i, j + 1));
        }
    for (uint32_t j = 0; j < np; ++j) tri(ring(nt - 1, j), (int32_t)bottom, ring(nt - 1, j + 1));
    return k == n_tris ? RT_OK : RT_ERR_STATE;
} RT_CATCH(nullptr)

} /* extern "C" */
