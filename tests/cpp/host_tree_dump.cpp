/*
 * host_tree_dump — TEST PROGRAM: the host builder's trees (rt_bvh.cpp) of a mesh, written to a
 * file for tests/tree_ref.py, on a machine without a GPU.  Links rt_bvh.cpp and this main only.
 *
 *   host_tree_dump verts.f32 idx.i32 out.bin [lights.f32 [light_weight]]
 *
 * The two trees are built and laid out as rt_set_mesh does (rt_mesh.cpp): the closest-hit tree
 * with cost weight 0; with lights, a second tree with the context's weight (RtBvh's default
 * unless given), its compressed nodes after the first tree's, inner links offset by the first
 * tree's node count and leaf slots by n_tris, its triangle records after the first tree's.
 * A tree that cannot be encoded drops the compressed nodes (and the second tree), as there.
 *
 * out.bin, little endian: 16 uint32
 *   [0] 0x44545452 "RTTD"  [1] n_tris  [2] n_nodes4  [3] n_nodes4_shadow  [4] shadow_root
 *   [5] n_records  [6] compressed  [7..9] n_hit, depth4, stack4 of the closest-hit tree
 *   [10..12] the same of the shadow tree (0 without one)  [13..15] 0
 * then nodes4 (32 floats x n_nodes4), nodes4q (16 dwords x (n_nodes4 + n_nodes4_shadow), if
 * compressed), tris (12 floats x n_records), and the shadow tree's full-precision nodes
 * (32 floats x n_nodes4_shadow, links offset like the compressed ones; rt_set_mesh keeps
 * none on the device).
 */
#include <cstdio>
#include <cstdlib>
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
    if (argc < 4) {
        fprintf(stderr, "usage: %s verts.f32 idx.i32 out.bin [lights.f32 [light_weight]]\n", argv[0]);
        return 2;
    }
    std::vector<float> verts, lights;
    std::vector<int32_t> idx;
    if (!read_all(argv[1], verts) || !read_all(argv[2], idx) || verts.size() % 3 || idx.size() % 3) {
        fprintf(stderr, "cannot read the mesh\n");
        return 2;
    }
    if (argc > 4 && (!read_all(argv[4], lights) || lights.size() % 3)) {
        fprintf(stderr, "cannot read the lights\n");
        return 2;
    }
    const uint32_t n_verts = (uint32_t)(verts.size() / 3), n_tris = (uint32_t)(idx.size() / 3);

    RtBvh b, sb;
    sb.light_centres = lights;
    if (argc > 5) sb.light_cost_weight = (float)atof(argv[5]);
    b.light_cost_weight = 0.0f;
    bool two = !sb.light_centres.empty() && sb.light_cost_weight > 0.0f && 2ull * n_tris < (1ull << 28);
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
                               0u,
                               0u,
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
