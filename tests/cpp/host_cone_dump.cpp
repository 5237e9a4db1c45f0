/*
 * host_cone_dump — TEST PROGRAM: host_tree_dump with the lights' radii, so that the shadow tree is
 * built with the cone split (rt_bvh.cpp never_occludes), on a machine without a GPU.  Links
 * rt_bvh.cpp and this main only.
 *
 *   host_cone_dump verts.f32 idx.i32 out.bin lights.f32
 *
 * lights.f32: 4 floats per light (centre, radius).  The trees are laid out as rt_set_mesh does
 * (rt_mesh.cpp) and out.bin is host_tree_dump's file, with two more header words:
 *   [13] subtree A's node, offset like the other links (0: no split)  [14] A's triangles
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "rt_internal.h"
#include "rt_quant.h"

namespace {

template <class T> bool read_all(const char *path, std::vector<T> &out)
{
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    fseek(f, 0, SEEK_END);
    const long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    out.resize(n > 0 ? (size_t)n / sizeof(T) : 0);
    const bool ok = n >= 0 && (size_t)n % sizeof(T) == 0 && fread(out.data(), sizeof(T), out.size(), f) == out.size();
    fclose(f);
    return ok;
}

template <class T> bool write_all(FILE *f, const std::vector<T> &v)
{
    return v.empty() || fwrite(v.data(), sizeof(T), v.size(), f) == v.size();
}

int32_t offset_link(int32_t code, uint32_t n_a, uint32_t n_tris)
{
    if (code == RT_EMPTY_CHILD) return code;
    if (code >= 0) return code + (int32_t)n_a;
    const uint32_t enc = (uint32_t)(~code);
    return ~(int32_t)((((enc >> 3) + n_tris) << 3) | (enc & 7u));
}

} // namespace

int main(int argc, char **argv)
{
    if (argc != 5) {
        fprintf(stderr, "usage: %s verts.f32 idx.i32 out.bin lights.f32\n", argv[0]);
        return 2;
    }
    std::vector<float> verts, lights;
    std::vector<int32_t> idx;
    if (!read_all(argv[1], verts) || !read_all(argv[2], idx) || verts.size() % 3 || idx.size() % 3) {
        fprintf(stderr, "cannot read the mesh\n");
        return 2;
    }
    if (!read_all(argv[4], lights) || lights.empty() || lights.size() % 4) {
        fprintf(stderr, "cannot read the lights\n");
        return 2;
    }
    const uint32_t n_verts = (uint32_t)(verts.size() / 3), n_tris = (uint32_t)(idx.size() / 3);

    RtBvh b, sb;
    for (size_t l = 0; l < lights.size() / 4; ++l) {
        sb.light_centres.insert(sb.light_centres.end(), &lights[4 * l], &lights[4 * l] + 3);
        sb.light_radii.push_back(lights[4 * l + 3]);
    }
    b.light_cost_weight = 0.0f;
    bool two = 2ull * n_tris < (1ull << 28);
    std::string err, err2;
    if (!rt_build_bvh(verts.data(), n_verts, idx.data(), n_tris, b, err)) {
        fprintf(stderr, "rt_build_bvh: %s\n", err.c_str());
        return 1;
    }
    const bool ok2 = two && rt_build_bvh(verts.data(), n_verts, idx.data(), n_tris, sb, err2);
    two = two && ok2 && !b.nodes4q.empty() && !sb.nodes4q.empty();

    std::vector<uint32_t> q4 = b.nodes4q;
    std::vector<float> tr = b.tris, f4s;
    const uint32_t n_a = b.n_nodes4;
    if (two) {
        q4.insert(q4.end(), sb.nodes4q.begin(), sb.nodes4q.end());
        for (size_t i = n_a; i < (size_t)n_a + sb.n_nodes4; ++i)
            for (int k = 0; k < 4; ++k) {
                uint32_t &w = q4[i * RT_QNODE_DWORDS + 12 + k];
                w = (uint32_t)offset_link((int32_t)w, n_a, n_tris);
            }
        tr.insert(tr.end(), sb.tris.begin(), sb.tris.end());
        f4s = sb.nodes4;
        for (uint32_t i = 0; i < sb.n_nodes4; ++i)
            for (int k = 0; k < 4; ++k) {
                int32_t c;
                memcpy(&c, &f4s[32ull * i + 24 + k], 4);
                c = offset_link(c, n_a, n_tris);
                memcpy(&f4s[32ull * i + 24 + k], &c, 4);
            }
    }
    const uint32_t head[16] = {0x44545452u,
                               n_tris,
                               n_a,
                               two ? sb.n_nodes4 : 0u,
                               two ? n_a : 0u,
                               (uint32_t)(tr.size() / 12),
                               q4.empty() ? 0u : 1u,
                               b.n_hit,
                               b.depth4,
                               b.stack4,
                               two ? sb.n_hit : 0u,
                               two ? sb.depth4 : 0u,
                               two ? sb.stack4 : 0u,
                               two && sb.cone_root4 ? n_a + sb.cone_root4 : 0u,
                               two ? sb.n_cone : 0u,
                               0u};
    FILE *f = fopen(argv[3], "wb");
    if (!f) {
        fprintf(stderr, "cannot write %s\n", argv[3]);
        return 2;
    }
    bool ok = fwrite(head, sizeof(head), 1, f) == 1;
    ok = ok && write_all(f, b.nodes4) && write_all(f, q4) && write_all(f, tr) && write_all(f, f4s);
    ok = fclose(f) == 0 && ok;
    return ok ? 0 : 2;
}
