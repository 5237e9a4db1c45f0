/*
 * rt_tri_rules.h — the two culling rules of rt_bvh.cpp on the device, term for term in binary64
 * on the float record the kernels read (v0, e1 = v1 - v0, e2 = v2 - v0 as float subtractions):
 * never_hit (no unit ray can accept the triangle) and never_occludes (no shadow query aimed at
 * the given lights can).  One copy for the refit (rt_refit.hip) and the device builders
 * (rt_build_gpu.hip).  Both are sound by the margins rt_bvh.cpp states (1.001, 0.999, 16u),
 * which dwarf any difference between the host's and the device's binary64 sqrt or division.
 */
#ifndef RT_TRI_RULES_H
#define RT_TRI_RULES_H

#include <hip/hip_runtime.h>

/* rt_bvh.cpp never_hit: from a record's float edges, or from the vertices */
__device__ __forceinline__ bool never_hit_edges(const float *e1, const float *e2)
{
    const double cx = (double)e2[1] * e1[2] - (double)e2[2] * e1[1];
    const double cy = (double)e2[2] * e1[0] - (double)e2[0] * e1[2];
    const double cz = (double)e2[0] * e1[1] - (double)e2[1] * e1[0];
    const double cr = sqrt(cx * cx + cy * cy + cz * cz);
    const double n1 = fabs((double)e1[0]) + fabs((double)e1[1]) + fabs((double)e1[2]);
    const double n2 = fabs((double)e2[0]) + fabs((double)e2[1]) + fabs((double)e2[2]);
    const double u = 1.0 / 16777216.0;
    const double bound = 1.001 * (cr + 16.0 * u * n1 * n2);
    return bound < 0.999 * (double)1e-4f;
}
__device__ __forceinline__ bool never_hit(const float *a, const float *p1, const float *p2)
{
    const float e1[3] = {p1[0] - a[0], p1[1] - a[1], p1[2] - a[2]};
    const float e2[3] = {p2[0] - a[0], p2[1] - a[1], p2[2] - a[2]};
    return never_hit_edges(e1, e2);
}

/* rt_bvh.cpp never_occludes from a record (a = v0 and its float edges): true when the rule's
   inequality holds for every one of the n_lights lights (centre.xyz, radius: 4 floats each). */
__device__ __forceinline__ bool never_occludes_edges(const float *a, const float *e1, const float *e2,
                                                     const float *__restrict__ lights, uint32_t n_lights)
{
    const double n[3] = {(double)e2[1] * e1[2] - (double)e2[2] * e1[1], (double)e2[2] * e1[0] - (double)e2[0] * e1[2],
                         (double)e2[0] * e1[1] - (double)e2[1] * e1[0]};
    const double cr = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
    const double n1 = fabs((double)e1[0]) + fabs((double)e1[1]) + fabs((double)e1[2]);
    const double n2 = fabs((double)e2[0]) + fabs((double)e2[1]) + fabs((double)e2[2]);
    const double u = 1.0 / 16777216.0;
    double cen[3], rt2 = 0.0;
    for (int k = 0; k < 3; ++k) cen[k] = (double)a[k] + ((double)e1[k] + (double)e2[k]) / 3.0;
    for (int v = 0; v < 3; ++v) {
        double d2 = 0.0;
        for (int k = 0; k < 3; ++k) {
            const double p = (double)a[k] + (v == 1 ? (double)e1[k] : v == 2 ? (double)e2[k] : 0.0);
            d2 += (p - cen[k]) * (p - cen[k]);
        }
        rt2 = fmax(rt2, d2);
    }
    const double rt = sqrt(rt2);
    for (uint32_t l = 0; l < n_lights; ++l) {
        double L[3], dist2 = 0.0, ln = 0.0;
        for (int k = 0; k < 3; ++k) {
            L[k] = (double)lights[4 * l + k] - cen[k];
            dist2 += L[k] * L[k];
            ln += L[k] * n[k];
        }
        const double dist = sqrt(dist2);
        const double reach = 1.001 * fabs((double)lights[4 * l + 3]) + rt;
        double maxcos = 1.0;
        if (reach < dist && cr > 0.0) {
            const double st = reach / dist, ct = sqrt(1.0 - st * st);
            const double cp = fmin(1.0, fabs(ln) / (dist * cr)), sp = sqrt(1.0 - cp * cp);
            if (cp < ct) maxcos = fmin(1.0, (cp * ct + sp * st) * (1.0 + 1e-9) + 1e-12);
        }
        const double bound = 1.001 * (cr * maxcos + 16.0 * u * n1 * n2);
        if (!(bound < 0.999 * (double)1e-4f)) return false;
    }
    return true;
}

#endif
