/*
 * pathtracer_rt.h — C-ABI drop-in boundary of the MI355X path tracer
 * (librtmi.so, built from pathtracer.cl_amd/csrc).
 *
 * It replaces the OpenCL host RayTracerCL (clrt/RayTracerCL.{h,cpp}) and the
 * device-agnostic RayTracer API (clrt/RayTracer.{h,cpp}) for the per-pixel
 * path-tracing kernels of clrt/ocl/raytracer.cl.  Plain pointers and sizes,
 * int status codes, no exceptions and no HIP/torch types in any signature.
 * One context per GPU; a context is not thread-safe (the reference is driven
 * from one GLUT thread, clrt/GlutCLWindow.cpp:136-227).
 *
 * Each entry point names the reference interface it replaces.
 */
#ifndef PATHTRACER_RT_H
#define PATHTRACER_RT_H

#include <stddef.h>
#include <stdint.h>

#include "rt_types.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rt_ctx rt_ctx;

/* Status codes (the reference throws cl::Error, RayTracerCL.cpp:102-107, :297-303). */
enum {
    RT_OK = 0,
    RT_ERR_ARG = -1,      /* bad argument (null pointer, zero size, out of range) */
    RT_ERR_HIP = -2,      /* a HIP runtime call failed; see rt_last_error() */
    RT_ERR_NO_SCENE = -3, /* render requested with no spheres set */
    RT_ERR_NO_MESH = -4,  /* triangle kernel requested with no mesh set */
    RT_ERR_ALLOC = -5,    /* host or device allocation failed */
    RT_ERR_STATE = -6,    /* inconsistent state (e.g. seed layout smaller than the frame) */
    RT_ERR_LIMIT = -7     /* input exceeds a device limit (e.g. BVH deeper than the traversal stack) */
};

/* Kernels of clrt/ocl/raytracer.cl. */
enum {
    RT_KERNEL_SPHERES = 0,    /* raytrace      raytracer.cl:46-104  (row-shifted seeds, sampleRate^2 samples) */
    RT_KERNEL_SPHERES_SS = 1, /* raytrace_ss   raytracer.cl:120-166 (one sample, unshifted seeds) */
    RT_KERNEL_TRIS = 2        /* raytrace_tris raytracer.cl:184-243 (mesh lit by the emissive spheres) */
};

/* Triangle traversal: the reference's linear loop (rtcommon.h:39-68) or a BVH
   (identical results: closest hit = minimum t, ties to the highest index).
   RT_TRAVERSAL_BVH is the 4-wide tree with compressed (8-bit quantised) 64-B
   nodes traversed per lane; RT_TRAVERSAL_BVH4F the same tree with full-precision
   128-B nodes (also the automatic fallback for meshes whose extent the quantised
   grid cannot encode).  Values 2 and 3 (a binary-tree and a wave-coherent packet
   traversal, measured slower) are retired: rt_set_traversal refuses them. */
enum {
    RT_TRAVERSAL_BVH = 0,
    RT_TRAVERSAL_LINEAR = 1,
    RT_TRAVERSAL_BVH4F = 4
};

/* rt_render flags */
enum {
    RT_OUT_DEVICE = 1, /* `out` is a device pointer on the context's GPU (else host memory) */
    RT_SEEDS_HALO = 2  /* the caller keeps the seed rows this tile reads current (seed-row halo,
                          below): permits progressive sphere frames on a tile */
};

/* Row-stripe tile of the frame owned by one rank (multi-GPU sharding).
   The frame's rows are cut into ceil(H / stripe_rows) stripes; stripe s belongs to rank
   stripe_owner[s], or, with stripe_owner NULL, to rank s % n_ranks (interleaved).  A rank's
   rows are rendered compacted in increasing y into `out` (rt_tile_rows() rows of W pixels).
   Seeds are always indexed in the global padded frame (raytracer.cl:207-209), so any
   partition renders the same bits.  NULL tile = full frame.  rt_partition_stripes makes a
   cost-balanced owner map. */
typedef struct rt_tile {
    uint32_t stripe_rows;
    uint32_t n_ranks;
    uint32_t rank;
    const uint32_t *stripe_owner; /* NULL, or ceil(H / stripe_rows) owners, each < n_ranks */
} rt_tile;

/* Ray accounting: one closest-hit query or one any-hit (shadow) query = 1 ray. */
typedef struct rt_counters {
    uint64_t rays_closest;
    uint64_t rays_shadow;
    uint64_t nodes_visited; /* BVH inner nodes fetched (counting launches only) */
    uint64_t tris_tested;   /* ray/triangle tests (counting launches only) */
    uint64_t leaves_visited; /* BVH leaves entered (counting launches only) */
    uint64_t lane_slots;     /* lanes x traversal-step rounds of the resumable (BVH) queries: SIMD
                                efficiency = (nodes_visited + leaves_visited) / lane_slots */
    uint64_t clocks_traversal; /* shader clocks waves spent in traversal rounds, summed over waves */
    uint64_t clocks_total;     /* shader clocks of the waves' whole lifetimes, summed over waves */
    uint64_t pixel_clocks_max; /* the costliest pixel: shader clocks from its refill to its write */
    uint64_t pixel_rays_max;   /* the most queries any one pixel needed */
    uint64_t pixel_steps_max;  /* the most traversal steps any one pixel needed */
    uint64_t rays_skipped;     /* shadow rays (counted in rays_shadow) answered without a
                                  traversal because the answer cannot change the pixel:
                                  tmax <= tmin, or cos(wi) <= 0 (rtcommon.h:93-95) */
    uint64_t clocks_shade;     /* shader clocks waves spent advancing paths (counting launches) */
    uint64_t pixels_long;      /* sample-split render: long chains (box pixels) run on their own stream */
} rt_counters;

/* ---- lifetime: RayTracerCL::RayTracerCL / init / ~RayTracerCL (RayTracerCL.cpp:52-145) ---- */
int rt_create(int device, rt_ctx **out);
int rt_destroy(rt_ctx *ctx);
const char *rt_last_error(const rt_ctx *ctx);
const char *rt_status_string(int status);

/* ---- scene: RayTracer::addSphere / clearSpheres (RayTracer.cpp:50-63) and the
   scene upload of RayTracerCL::rayTrace (RayTracerCL.cpp:251-264) ---- */
int rt_set_spheres(rt_ctx *ctx, const rt_sphere *spheres, uint32_t n);

/* ---- mesh: the tri_verts / tri_vert_idx / n_tris kernel arguments of
   raytrace_tris (raytracer.cl:184-188); the context builds the BVH (the host build's cost area
   leans toward the emissive spheres of the last rt_set_spheres; a later rt_set_spheres keeps the
   tree: culling only, no result depends on it). ---- */
int rt_set_mesh(rt_ctx *ctx, const float *verts_xyz, uint32_t n_verts, const int32_t *idx, uint32_t n_tris);
/* BVH statistics of the current mesh. */
typedef struct rt_mesh_stats {
    uint32_t n_tris;
    uint32_t n_nodes2, depth2; /* binary tree */
    uint32_t n_nodes4, depth4; /* 4-wide tree */
    uint32_t stack4;           /* worst-case traversal stack of the 4-wide tree */
    double build_seconds;
    uint32_t builder; /* RT_BUILD_HOST, RT_BUILD_GPU or RT_BUILD_GPU_PLOC */
    uint32_t n_tris_tree; /* triangles in the tree: the host build (and a device build with
                             RT_BUILD_OPT_LIGHTS) leaves out those no ray can hit (|det| < 1e-4
                             for every unit direction, geometryFuncs.h:167) */
    uint32_t n_nodes4_shadow; /* the shadow queries' 4-wide tree (host build with lights: its cost
                                 area leans toward them); 0: they walk the closest-hit tree */
    uint32_t cone_root;   /* the lights' cone split of the shadow tree (host build, or a device build with
                             RT_BUILD_OPT_LIGHTS; RT_LIGHT_CONE): the node
                             of the subtree over the triangles that can occlude the lights it was built for —
                             the shadow queries start there while the lights and the tree stay as they were
                             (rt_render_info.shadow_start); 0: no split */
    uint32_t n_tris_cone; /* that subtree's triangles */
    uint32_t collapse;    /* RT_COLLAPSE_*: how the binary tree became the 4-wide one (a host build:
                             RT_COLLAPSE_SAH) */
} rt_mesh_stats;
/* BVH builder used by the next rt_set_mesh: the host binned-SAH build (default: the best
   trees), the GPU build (LBVH over Morton codes, collapsed on the device: seconds-to-
   milliseconds for large meshes, somewhat slower traversal), or the GPU PLOC build (the same
   sorted order, merged bottom-up by surface area in rounds of mutual nearest neighbours: a
   few times the LBVH's build time, trees nearer the host build's).  Both GPU builds make one
   tree and keep every triangle unless rt_set_build_options says otherwise.  Results are
   identical under all three. */
enum { RT_BUILD_HOST = 0, RT_BUILD_GPU = 1, RT_BUILD_GPU_PLOC = 2 };
int rt_set_builder(rt_ctx *ctx, int builder);
/* Options of the device builders for the next rt_set_mesh (default 0: one tree over every
   triangle).  RT_BUILD_OPT_LIGHTS: what the host build does around its trees, done on the
   device — the triangles no unit ray can accept are left out (n_tris_tree), and the shadow
   queries get a second tree (n_nodes4_shadow) whose root has exactly two children, A over the
   triangles that can occlude the lights of the last rt_set_spheres (cone_root, n_tris_cone) and B
   over the rest; without such a split (no lights, a part of at most one leaf, nodes the
   compressed form cannot hold, rt_set_mesh_dynamic) the build makes one tree.  The host builder
   ignores the options.  The mesh remembers them as it remembers its builder: a rebuild inside
   rt_update_mesh uses the mesh's own, and after a refit of such a mesh the split is checked in
   the new pose and kept while it still holds.  Culling only: no result bit depends on it.
   Unknown bits: RT_ERR_ARG, the options stay as they were. */
enum { RT_BUILD_OPT_LIGHTS = 1 };
int rt_set_build_options(rt_ctx *ctx, uint32_t opts);
int rt_get_build_options(const rt_ctx *ctx, uint32_t *opts);
/* How the device builders collapse their binary tree to the 4-wide one, for the next rt_set_mesh.
   RT_COLLAPSE_GREEDY (default): the inner child of largest area is expanded until there are four,
   and every subtree of at most 4 triangles becomes one leaf.  RT_COLLAPSE_SAH: the host build's
   rule — by dynamic programming over the binary tree every node becomes a leaf, a wide node of
   its own or is dissolved into its parent's children, whichever costs fewer area-weighted
   traversal steps: more and smaller nodes, a stack a few entries deeper.  The
   host builder ignores the mode; the mesh remembers it as it remembers its builder (a rebuild
   inside rt_update_mesh uses the mesh's own; rt_mesh_stats.collapse).  Culling only: no result
   bit depends on it.  Any other value: RT_ERR_ARG, the mode stays as it was. */
enum { RT_COLLAPSE_GREEDY = 0, RT_COLLAPSE_SAH = 1 };
int rt_set_collapse(rt_ctx *ctx, int mode);
int rt_get_collapse(const rt_ctx *ctx, int *mode);
int rt_mesh_info(const rt_ctx *ctx, rt_mesh_stats *out);

/* ---- a moving mesh: new positions for the vertices of the last rt_set_mesh (same count, same
   indices), by a refit of both trees on the device — the records, the boxes, the compressed
   planes and the normal boxes recomputed from the trees' own links; no build, no upload of
   nodes.  Synchronous.  Every result afterwards is bit for bit what a fresh rt_set_mesh with the
   new vertices gives; rt_mesh_info's numbers stay those of the build.  Errors (RT_ERR_NO_MESH;
   RT_ERR_ARG for another vertex count or a non-finite coordinate) leave the previous mesh as it
   was.  The call rebuilds instead, as rt_set_mesh with the kept indices and the mesh's own
   builder, when a triangle the host builder left out of the tree (no unit ray could hit it) can
   now be hit, or when the compressed form stops / starts holding every node.
   rt_set_mesh_dynamic(ctx, 1) makes the next host build keep every triangle, so that later
   updates always refit (the tree then holds the never-hit triangles too).  area_ratio tells how
   far the refitted boxes have grown since the build: the sign to call rt_set_mesh again. ---- */
enum { RT_MESH_VERTS_DEVICE = 1 }; /* flags: verts_xyz is a device pointer */
enum { RT_MESH_UPDATE_REFIT = 1, RT_MESH_UPDATE_REBUILT = 2 };
enum { RT_REFIT_OK = 0, RT_REFIT_NEWLY_HITTABLE = 1, RT_REFIT_ENCODING = 2 };
typedef struct rt_mesh_update_info {
    uint32_t action;         /* REFIT or REBUILT */
    uint32_t reason;         /* why rebuilt, else RT_REFIT_OK */
    uint32_t newly_hittable; /* triangles left out of the tree that a unit ray can now hit */
    uint32_t now_unhittable; /* triangles in the tree that a unit ray could hit when it was built and none can
                                now (they stay) */
    float area_ratio;        /* closest-hit tree: sum of child-box half-areas now / at its build */
    float ms;                /* device time of the refit kernels (HIP events); 0 when rebuilt */
} rt_mesh_update_info;
int rt_update_mesh(rt_ctx *ctx, const float *verts_xyz, uint32_t n_verts, int flags);
int rt_last_mesh_update(const rt_ctx *ctx, rt_mesh_update_info *out);
int rt_set_mesh_dynamic(rt_ctx *ctx, int on); /* for the next rt_set_mesh */
/* The vertices of the current mesh as the trees hold them: those of the last successful
   rt_set_mesh / rt_update_mesh.  3 * n_verts floats; flags: RT_OUT_DEVICE = out is a device pointer.
   RT_ERR_NO_MESH without a mesh; RT_ERR_ARG for a null pointer or another vertex count. */
int rt_mesh_pose(rt_ctx *ctx, float *out_verts_xyz, uint32_t n_verts, int flags);

/* ---- camera: RayTracer::setCameraMatrix / setCameraSpherical / setFoVAngle
   (RayTracer.h:56-60, RayTracer.cpp:24-47); the Camera struct is derived per
   frame width exactly as RayTracerCL::updateCLCamera (RayTracerCL.cpp:178-215). ---- */
int rt_set_view_matrix(rt_ctx *ctx, const float m_colmajor[16]);
int rt_set_camera_spherical(rt_ctx *ctx, float tx, float ty, float tz, float elevation_deg, float azimuth_deg,
                            float distance);
int rt_set_fov(rt_ctx *ctx, float fov_deg);
/* Explicit Camera override (fixtures); cleared by the three calls above. */
int rt_set_camera(rt_ctx *ctx, const rt_camera *cam);
/* Host helper: the Camera the reference would upload for this setup and width. */
int rt_camera_spherical(float tx, float ty, float tz, float elevation_deg, float azimuth_deg, float distance,
                        float fov_deg, uint32_t width, rt_camera *out);

/* ---- settings: RayTracer::setSampleRate / setMaxPathDepth (RayTracer.h:62-66) ---- */
int rt_set_params(rt_ctx *ctx, uint32_t sample_rate, uint32_t max_depth);
int rt_set_traversal(rt_ctx *ctx, int traversal);

/* ---- RNG seeds: RayTracerCL::updateSeedBuffer (RayTracerCL.cpp:147-171).
   Work-group height ndY fixes the padded height (RayTracerCL.cpp:114-116,
   :229-232; 8 = a 256-item work-group on AMD GPUs, the default). ---- */
int rt_set_ndrange(rt_ctx *ctx, uint32_t nd_y);
/* Allocate a Wpad x Hpad layout filled from the context's glibc-rand() stream
   (glibc TYPE_3 random(), default seed 1 — no srand in the reference). */
int rt_set_seed_layout(rt_ctx *ctx, uint32_t wpad, uint32_t hpad);
/* Replace the seeds: count == 2 * Wpad * Hpad (x plane then y plane). */
int rt_set_seeds(rt_ctx *ctx, const uint32_t *seeds, size_t count);
int rt_get_seeds(const rt_ctx *ctx, uint32_t *out, size_t count);
int rt_seed_layout(const rt_ctx *ctx, uint32_t *wpad, uint32_t *hpad);
/* Seed-row halo for multi-GPU progressive sphere frames.  raytrace reads and writes
   seed row (y + progressive) % Hpad for pixel row y (get_seed / put_seed,
   raytracer.cl:20-30), so between frames one seed row per stripe boundary moves to
   the neighbouring rank.  These copy whole rows (both planes) of the context's seed
   layout to / from a packed buffer laid out [plane][i][x] (2 * n * Wpad words);
   `buf` is a device pointer with RT_OUT_DEVICE in flags, else host memory.  The
   rows to move are planned by pathtracer.cl_amd/dist.py (SeedHalo). */
int rt_pack_seed_rows(rt_ctx *ctx, const uint32_t *rows, uint32_t n, uint32_t *buf, int flags);
int rt_unpack_seed_rows(rt_ctx *ctx, const uint32_t *rows, uint32_t n, const uint32_t *buf, int flags);
/* glibc rand() stream restated (tests compare it with libc's own rand()). */
int rt_glibc_rand_fill(uint32_t seed, uint32_t *out, size_t count, uint32_t skip);

/* ---- render: RayTracerCL::rayTrace(cl_mem*, W, H, progression) (RayTracerCL.cpp:217-307).
   progression 0 overwrites; p > 0 mixes with weight 1/p (GlutCLWindow.cpp:144-158).
   Pads the frame, (re)creates seeds on a size change and refreshes the camera
   exactly as the reference does, then launches and waits (finish()). ---- */
int rt_render(rt_ctx *ctx, float *out_rgba, uint32_t width, uint32_t height, uint32_t progression, int kernel,
              const rt_tile *tile, int flags);
/* Same, enqueued on `hip_stream` (a hipStream_t, or NULL = the context stream), no wait. */
int rt_render_async(rt_ctx *ctx, float *out_rgba, uint32_t width, uint32_t height, uint32_t progression,
                    int kernel, const rt_tile *tile, int flags, void *hip_stream);
int rt_synchronize(rt_ctx *ctx);
/* Blocking readback of the last render's framebuffer (W x rows x 4 floats) into host
   memory: the non-sharing display path, enqueueReadBuffer(clPBOBuff, CL_TRUE, ...)
   into the mapped PBO (GlutCLWindow.cpp:214-225).  Valid while the buffer passed to
   that render (device framebuffers) is alive.  n_floats = capacity of `host`. */
int rt_read(rt_ctx *ctx, float *host, size_t n_floats);
/* Rows of `height` owned by `tile` (NULL: height). */
uint32_t rt_tile_rows(uint32_t height, const rt_tile *tile);
/* Cost-balanced partition of a W x H raytrace_tris frame's row stripes over n_ranks for the
   context's current camera, mesh and lights (the multi-GPU split; the reference renders on one
   device, RayTracerCL.cpp:217-307).  A probe of the whole frame — one camera ray per pixel
   through the compressed tree, and its shadow rays — counts per stripe the pixels whose camera
   ray misses the mesh (box pixels: the long serial chains of a tile) and the
   probe's traversal steps of the others; the stripes are dealt largest cost first to the least
   loaded rank (LPT; ties to the lower stripe and rank index).  Deterministic: every rank
   computes the same map from the same scene.  Cached per view (camera, mesh, lights, frame
   shape).  owner: ceil(H / stripe_rows) entries.  *recomputed (may be NULL) = 1 when the probe
   ran, 0 when the cached map was returned. */
int rt_partition_stripes(rt_ctx *ctx, uint32_t width, uint32_t height, uint32_t stripe_rows, uint32_t n_ranks,
                         uint32_t *owner, int *recomputed);

/* ---- instrumentation ---- */
int rt_get_counters(const rt_ctx *ctx, rt_counters *out); /* of the last completed render (or counting rt_trace_rays call) */
int rt_set_counting(rt_ctx *ctx, int enable);             /* count nodes/tris in the next renders */
/* Running totals over every render since the context was created or the totals were last reset
   (renders enqueued back to back with rt_render_async overwrite each other's rt_get_counters;
   their totals are kept on the device): waits for the context's renders, then sums of the summed
   counters, maxima of the per-pixel maxima (pixels_long: 0), *renders = renders counted.
   reset != 0 zeroes the totals after reading them.  RT_ERR_STATE if a sample-split defect guard
   fired in any of those renders (rt_synchronize reports only the last one's). */
int rt_counter_totals(rt_ctx *ctx, rt_counters *sum, uint64_t *renders, int reset);
/* Device time of the last render's kernel (HIP events on the launch stream), ms. */
int rt_last_kernel_ms(const rt_ctx *ctx, float *ms);
/* The same time split at the start of the main path kernel: the camera-ray candidate-list
   pre-pass of a triangle render (0 without one), then k_tris (+ a sample-split render's seed
   passes and in-order sums), ms. */
int rt_last_kernel_split_ms(const rt_ctx *ctx, float *prepass_ms, float *main_ms);

/* What the last render did beyond the reference's launch (the triangle kernel's own
   machinery; none of it changes a result bit). */
typedef struct rt_render_info {
    uint32_t kernel;           /* RT_KERNEL_* of the last render */
    uint32_t traversal;        /* internal traversal kind of a triangle render */
    uint32_t grid_blocks;      /* persistent grid of the main kernel */
    uint32_t lists;            /* 1: camera-ray candidate lists were built and used */
    uint64_t list_capacity;    /* list-area records (48 B each) reserved for the render */
    uint64_t list_records;     /* records the pixels' lists took (read on the first call) */
    uint32_t list_pixels_tree; /* pixels without a list (over RT_LIST_MAX candidates, a deep
                                  frustum stack, or the area full): their camera rays took the tree */
    uint32_t pixels_long;      /* sample-split render: long chains (box pixels) run on their own stream */
    uint32_t schedule_rebuilt; /* 1: the cost probe, LPT order and pixel classes were recomputed
                                  (camera, mesh, frame, tile or parameters changed) */
    uint32_t lists_rebuilt;    /* 1: the lists were built for this render (0: the previous render's,
                                  same camera, mesh, frame and tile, were reused) */
    double schedule_host_ms;   /* host time spent enqueueing / sizing the schedule this render */
    uint32_t split_chunks;     /* sample-split render (a tile with few pixels per lane): chunks per
                                  pixel, each an independent task seeded by the seed pass; 0: whole pixels */
    uint32_t split_coop;       /* lanes per query of the long chains' seed pass (4: coop_round; 0: one) */
    uint32_t split_guard;      /* read after completion: a defect guard of the long chains' seed pass
                                  fired (record index out of range, group stack overflow, query round
                                  bound); rt_synchronize then fails with RT_ERR_STATE */
    uint32_t split_spec;       /* 1: the mesh pixels' chunk seeds were jumped ahead from their frame
                                  seeds (no seed pass for them; pixels near a silhouette run as long chains) */
    uint32_t split_repaired;   /* read after completion: speculated pixels whose camera rays missed the
                                  mesh after all, re-rendered by the repair pass (seed pass + chunks) */
    uint32_t split_hit_depth;  /* 1: the long chains' chunk tasks answered their box segments' closest-hit
                                  queries from the seed pass's per-sample mesh-hit depths (no traversal) */
    uint32_t schedule_measured; /* 1: the queue's tiles were ordered by the view's previous frame's measured
                                   per-pixel costs (its traversal steps), not by the cost probe */
    uint32_t schedule_pilot;    /* 1: a view's first frame, ordered by the per-pixel costs of a pilot render of
                                   a few samples per pixel (scratch seeds and framebuffer), not by the probe */
    uint32_t shadow_start;      /* the node the shadow queries started at: rt_mesh_stats.cone_root, or the shadow
                                   tree's root (the closest-hit tree's, 0, without one) */
} rt_render_info;
int rt_last_render_info(rt_ctx *ctx, rt_render_info *out);
/* The long chains of the last sample-split render (pixels_long of them: tile-local y * W + x, the
   order of their slots), the pixels whose seed pass ran on the second stream with split_coop lanes
   per query.  Copies min(cap, *n) entries; *n = pixels_long.  Diagnostics and parity tests. */
int rt_last_long_chains(rt_ctx *ctx, uint32_t *out, uint32_t cap, uint32_t *n);
/* The camera-ray candidate lists of the last triangle render, per pixel (tile-local y * W + x): the
   records of its list, 0 for a pixel no triangle can be hit through, 0xffff for a pixel without a
   list (its camera rays take the tree).  Copies min(cap, *n) entries; *n = the render's pixels, 0
   when it used no lists.  Diagnostics and parity tests. */
int rt_last_list_counts(rt_ctx *ctx, uint16_t *out, uint32_t cap, uint32_t *n);
/* The current mesh's trees as the kernels read them, copied from the device: the full-precision
   4-wide nodes of the closest-hit tree (32 floats each), the compressed nodes of both trees (16
   dwords each, the shadow tree's from shadow_root on, links and record slots already offset) and
   the triangle records the trees' leaves refer to (12 floats each).  A NULL array is not copied;
   *layout is always filled.  RT_ERR_NO_MESH without a mesh, RT_ERR_STATE when nodes4q is asked
   for and the mesh has no compressed nodes.  Diagnostics and tests (tests/tree_ref.py). */
typedef struct rt_tree_layout {
    uint32_t n_nodes4;        /* closest-hit tree */
    uint32_t n_nodes4_shadow; /* 0: one tree */
    uint32_t shadow_root;     /* index of the shadow tree's root in the compressed array */
    uint32_t n_records;       /* triangle records the trees refer to */
    uint32_t compressed;      /* 1: compressed nodes exist */
} rt_tree_layout;
int rt_mesh_tree(rt_ctx *ctx, rt_tree_layout *layout, float *nodes4, uint32_t *nodes4q, float *tris);

/* ---- ray queries for hit-index parity (rtcommon.h:39-52 / :59-68 semantics).
   Host arrays; any_hit=0: out_idx = closest triangle (-1 none), out_t = its t;
   any_hit=1: out_idx = 1 if occluded in (tmin, tmax). ---- */
int rt_trace_rays(rt_ctx *ctx, const rt_ray *rays, uint32_t n, int any_hit, int32_t *out_idx, float *out_t);

/* ---- first-hit feature buffers and the display denoiser.  Nothing in the reference corresponds
   to them (raytracer.cl:220 leaves a TODO at the camera ray); their arithmetic is pinned in
   DESIGN.md §4.9 under the model of rt_math.h, so both are reproducible to the bit.  They
   serve the DISPLAYED image only: no call here changes any render state (seeds, schedule / list /
   pilot caches, counters, rt_last_kernel_ms, rt_last_render_info, rt_read's framebuffer), and the
   accumulation buffer a progressive render mixes into is never written.  `flags` takes
   RT_OUT_DEVICE only: with it every buffer of the call is a device pointer on the context's GPU,
   without it every buffer is host memory and the library stages them.  On any stream the calls
   order themselves after the context's pending render, and the next render after them.
   The features cover the whole frame — there is no rt_tile: in a multi-GPU run the root computes
   them itself for the gathered frame. ---- */
/* surface ids in a feature buffer: >= 0 triangle index (the caller's numbering, as rt_trace_rays) */
enum { RT_FEAT_BOX = -1, RT_FEAT_NONE = -2, RT_FEAT_SPHERE0 = -16 /* sphere s: RT_FEAT_SPHERE0 - s */ };
/* The Camera rt_render would use for a frame of this width: the explicit override, or the one
   derived from the view matrix and the field of view (RayTracerCL::updateCLCamera). */
int rt_get_camera(const rt_ctx *ctx, uint32_t width, rt_camera *out);
/* host only: the pixel-centre camera rays of a W x H frame, row-major y*W+x: raytracer.cl:221-224
   with the stratified draw replaced by 0.5; o = position, tmin = 1e-4f, tmax = INFINITY,
   propagation 1, extinction 0, diffuse flag 0. */
int rt_primary_rays(const rt_camera *cam, uint32_t width, uint32_t height, rt_ray *out);
/* The first hit of every pixel-centre ray under the context's current camera (derived for
   `width`), as the kernel's first path segment finds it: RT_KERNEL_TRIS the mesh (closest hit,
   ties to the highest index; N = normalize(cross(e2, e1)), never flipped) then the box;
   RT_KERNEL_SPHERES / _SS the spheres (strict interval, lowest index on ties) then the box.
   feat: 2 planes of W*H float4; plane 0 = (Px,Py,Pz,t), plane 1 = (Nx,Ny,Nz, id as int32 bits);
   a pixel that meets nothing: id RT_FEAT_NONE, P = N = 0, t = INFINITY.  The same bits under
   every rt_set_traversal mode and both builders.  RT_ERR_NO_SCENE / RT_ERR_NO_MESH as rt_render. */
int rt_render_features(rt_ctx *ctx, float *feat, uint32_t width, uint32_t height, int kernel, int flags);
int rt_render_features_async(rt_ctx *ctx, float *feat, uint32_t width, uint32_t height, int kernel, int flags,
                             void *hip_stream);
/* Edge-avoiding a-trous wavelet filter (Dammertz et al. 2010; plane-distance position term) of an
   RGBA32F frame guided by its feature buffer: `iterations` passes (1..8) of a 5x5 B3-spline kernel
   at tap distance 1 << pass; each tap weighted by exp(-(|dc|^2/sc^2 + |dN|^2/sn^2 + (dP.N)^2/sp^2)),
   the colour tolerance sc halving every pass.  A sigma of +INFINITY switches its term off; a sigma
   <= 0 or NaN is RT_ERR_ARG.  Alpha is copied.  out_rgba == in_rgba is allowed (no other overlap);
   in_rgba (otherwise) and feat are never written; intermediate passes live in scratch the context
   owns.  Inputs are assumed finite, apart from the t of RT_FEAT_NONE pixels, which the filter
   does not read. */
typedef struct rt_denoise_params {
    uint32_t iterations;
    float sigma_color, sigma_normal, sigma_plane;
} rt_denoise_params;
int rt_denoise_defaults(rt_denoise_params *p); /* 5, 2.0f, 0.3f, 0.1f */
int rt_denoise(rt_ctx *ctx, const float *in_rgba, const float *feat, float *out_rgba, uint32_t width, uint32_t height,
               const rt_denoise_params *params, int flags);
int rt_denoise_async(rt_ctx *ctx, const float *in_rgba, const float *feat, float *out_rgba, uint32_t width,
                     uint32_t height, const rt_denoise_params *params, int flags, void *hip_stream);
/* Device time of the last feature kernel / of all passes of the last denoise (HIP events of their
   own, apart from rt_last_kernel_ms), ms. */
int rt_last_features_ms(const rt_ctx *ctx, float *ms);
int rt_last_denoise_ms(const rt_ctx *ctx, float *ms);

/* ---- temporal reprojection of the displayed frame across camera moves.  The
   rules of the feature / denoise calls above hold: display only, no render state is changed, the
   accumulation buffer is only read, `flags` takes RT_OUT_DEVICE only, the same stream ordering, and
   arithmetic that a float32 restatement reproduces to the bit.  A history is a displayed RGBA32F
   frame with, per pixel, the number of frames it averages (`*_len`, one plane of W*H floats; 0: none).
   The scene is assumed static between the two views, both frames W x H; the caller drops its
   history on a reshape or a scene change.  Inputs are assumed finite where they are read. ---- */
typedef struct rt_reproject_params {
    float plane_tol;   /* tap q lies on pixel p's surface when |(P_q - P_p).N_p| <= plane_tol * t_p */
    float normal_min;  /* ... and N_q.N_p >= normal_min */
    float max_history; /* cap of the carried history length, in frames */
} rt_reproject_params;
int rt_reproject_defaults(rt_reproject_params *p); /* 0.01f, 0.9f, 32.0f */
/* Backward reprojection, once per view change: for every pixel p of the new view (cur_feat, as
   rt_render_features wrote it) solve P_p - prev_cam.position = s (view + a right + b up) (the
   general 3x3 solve, prev_cam need not be orthogonal); fx = a + W/2 - 0.5, fy = b + H/2 - 0.5 is its
   place in the previous frame (the inverse of rt_primary_rays).  No history (out rgb = 0, out_len =
   0) when p met nothing, s <= 0, the determinant is 0, or the place is not finite or has no tap
   inside the frame.  Otherwise the four bilinear taps (floor fx + {0,1}, floor fy + {0,1}); tap q
   counts when it is inside the frame, prev_len[q] > 0, q met a surface of p's class (any two
   triangles match, a sphere only itself, the box only the box) and passes the two tests above:
   out rgb = sum(w c_q) / wsum, out_len = min(sum(w len_q) / wsum, max_history), out a = 0; no
   counting tap (wsum = 0): no history.  plane_tol < 0 or NaN, normal_min NaN, max_history < 1 or
   NaN: RT_ERR_ARG; plane_tol +INFINITY switches that test off.  out_* may not be prev_*
   (RT_ERR_ARG); no input is written. */
int rt_reproject(rt_ctx *ctx, const float *prev_rgba, const float *prev_len, const float *prev_feat,
                 const rt_camera *prev_cam, const float *cur_feat, float *out_rgba, float *out_len, uint32_t width,
                 uint32_t height, const rt_reproject_params *params, int flags);
int rt_reproject_async(rt_ctx *ctx, const float *prev_rgba, const float *prev_len, const float *prev_feat,
                       const rt_camera *prev_cam, const float *cur_feat, float *out_rgba, float *out_len, uint32_t width,
                       uint32_t height, const rt_reproject_params *params, int flags, void *hip_stream);
/* Every displayed frame: blend the carried history (h, m) with the accumulation buffer c of n_cur
   frames (max(progression, 1): a progressive render's frame 0 is overwritten by frame 1).  Where
   m > 0: out rgb = h + (c - h) (n / (n + m)), out_len = min(n + m, max_history); elsewhere out rgb =
   c's bits, out_len = min(n, max_history).  out a = c.a.  out_rgba == hist_rgba and out_len ==
   hist_len are allowed; cur_rgba is never written (out_rgba == cur_rgba: RT_ERR_ARG).  n_cur < 1 or NaN, max_history < 1 or NaN:
   RT_ERR_ARG. */
int rt_temporal_merge(rt_ctx *ctx, const float *hist_rgba, const float *hist_len, const float *cur_rgba, float n_cur,
                      float max_history, float *out_rgba, float *out_len, uint32_t width, uint32_t height, int flags);
int rt_temporal_merge_async(rt_ctx *ctx, const float *hist_rgba, const float *hist_len, const float *cur_rgba,
                            float n_cur, float max_history, float *out_rgba, float *out_len, uint32_t width,
                            uint32_t height, int flags, void *hip_stream);
/* Device time of the last reprojection kernel and of the last merge kernel (HIP events of their
   own), ms; either pointer may be NULL.  RT_ERR_STATE when a kernel asked for has not run. */
int rt_last_reproject_ms(const rt_ctx *ctx, float *reproject_ms, float *merge_ms);

/* ---- lag-adaptive trust of the carried history: per pixel, is the radiance that
   rt_reproject carried still true?  Display only, under the rules of the calls above. ---- */
typedef struct rt_trust_params {
    float tolerance;                 /* standard deviations the window means may differ by; +INFINITY: all is trusted */
    float sigma_normal, sigma_plane; /* the window's feature weights, as rt_denoise_params */
} rt_trust_params;
int rt_trust_defaults(rt_trust_params *p); /* 1.5f, 0.3f, 0.1f */
/* Every displayed frame of a view that carries history, before rt_temporal_merge: hist_rgba /
   hist_len the carried history as rt_reproject wrote it for the current view, cur_rgba the
   accumulation buffer of n_cur = max(progression, 1) frames, feat the current view's features
   (unwarped).  out_len, one plane of W*H floats: the history length each pixel still deserves, to be
   passed to rt_temporal_merge as hist_len.  Per pixel p with m = hist_len[p]: !(m > 0): 0; p met
   nothing: m.  Otherwise over the 7x7 window at unit distance (dy outer, dx inner; a tap counts when
   it is inside the frame, has hist_len > 0, met a surface, and that surface is of p's class as in
   rt_reproject), with w = exp(-(|dN|^2/sn^2 + (dP.N)^2/sp^2)), Lc = lum(cur_q), Lh = lum(hist_q):
   mc, mh the weighted means of Lc, Lh; vc, vh their weighted variances (max(., 0)); ne = sum(w^2) /
   sum(w)^2.  ne > 0.5 (fewer than two effective taps): m.  v = max(vc, vh max(m, 1) / n_cur);
   z2 = (mc - mh)^2 / (v ne (1 + n_cur / m) + 1e-12); out = m where !(z2 > tolerance^2), else
   m tolerance^2 / z2.  (max(a, b) = a > b ? a : b.)  out_len == hist_len is allowed (no other
   overlap); no other input is written.  tolerance +INFINITY returns hist_len bit for bit.
   tolerance <= 0 or NaN, a sigma <= 0 or NaN, n_cur < 1 or NaN, null pointers, an empty frame:
   RT_ERR_ARG. */
int rt_history_trust(rt_ctx *ctx, const float *hist_rgba, const float *hist_len, const float *cur_rgba, float n_cur,
                     const float *feat, float *out_len, uint32_t width, uint32_t height, const rt_trust_params *params,
                     int flags);
int rt_history_trust_async(rt_ctx *ctx, const float *hist_rgba, const float *hist_len, const float *cur_rgba, float n_cur,
                           const float *feat, float *out_len, uint32_t width, uint32_t height,
                           const rt_trust_params *params, int flags, void *hip_stream);
/* Device time of the last trust kernel (HIP events of its own), ms; RT_ERR_STATE before a first run. */
int rt_last_trust_ms(const rt_ctx *ctx, float *ms);

/* ---- carrying the displayed frame across rt_update_mesh: the current features
   rewritten into an earlier pose of the mesh, for rt_reproject's cur_feat. ---- */
/* cur_feat as rt_render_features wrote it for the CURRENT pose; prev_verts_xyz: an earlier pose of the
   same mesh (n_verts as the mesh's).  out_feat: the same two planes with every mesh pixel's P and N
   replaced by those of the same material point in the earlier pose — the hit point's barycentrics
   (u, v) in its triangle (id) of the current pose (rt_mesh_pose), unclamped, then P' = (a' + e1' u) +
   e2' v and N' = normalize(cross(e2', e1')) from the earlier vertices; t and id stay.  Pixels of the
   box, a sphere or nothing (id < 0) are copied bit for bit.  A mesh pixel becomes "no surface" (P = N
   = 0, t = INFINITY, id RT_FEAT_NONE: rt_reproject gives it no history) when its id is not below the
   triangle count, an index of its triangle is outside [0, n_verts), either triangle is degenerate, or
   P' / N' is not finite.  Display only: the rules of the feature / denoise / reproject calls (no
   render state changed, flags takes RT_OUT_DEVICE only and then every buffer incl. prev_verts_xyz is
   a device pointer, the same stream ordering).  out_feat == cur_feat is allowed (no other overlap).
   RT_ERR_NO_MESH without a mesh; RT_ERR_ARG for null pointers, an empty frame or another n_verts. */
int rt_warp_features(rt_ctx *ctx, const float *cur_feat, const float *prev_verts_xyz, uint32_t n_verts,
                     float *out_feat, uint32_t width, uint32_t height, int flags);
int rt_warp_features_async(rt_ctx *ctx, const float *cur_feat, const float *prev_verts_xyz, uint32_t n_verts,
                           float *out_feat, uint32_t width, uint32_t height, int flags, void *hip_stream);
/* Device time of the last warp kernel (HIP events of its own), ms; RT_ERR_STATE before a first run. */
int rt_last_warp_ms(const rt_ctx *ctx, float *ms);

/* ---- carrying the displayed frame across rt_set_spheres: the sphere twin of
   rt_warp_features.  cur_feat: the features of the current view under the context's current spheres
   (the last rt_set_spheres; rt_render_features with a sphere kernel).  out_feat: the same buffer with
   every sphere pixel's hit point put back where that sphere stood in prev_spheres (n_prev records; sphere
   i of both lists is the same object).  Per pixel with (N, id) of plane 1: a mesh pixel, the box, nothing
   or any other id above RT_FEAT_SPHERE0 is copied bit for bit.  Sphere s = RT_FEAT_SPHERE0 - id: not
   below both counts, "no surface" (P = N = 0, t = INFINITY, id RT_FEAT_NONE: rt_reproject gives it no
   history); centre and radius of current and earlier sphere s equal in all four words' bits (the
   material is not compared), copied bit for bit; otherwise P' = (C'.x + N.x r', C'.y + N.y r', C'.z +
   N.z r') with (C', r') the earlier sphere, every product and sum one rounded float32 operation, and N, t
   and id stay — or "no surface" when r' is not positive and finite or a component of P' is not finite.
   Display only, under rt_warp_features' rules: no render state changed, flags takes RT_OUT_DEVICE only
   and then every buffer incl. prev_spheres is a device pointer, the same stream ordering.  n_prev == 0
   is legal (prev_spheres may then be NULL): every sphere pixel becomes "no surface".  out_feat ==
   cur_feat is allowed (no other overlap).  RT_ERR_NO_SCENE without current spheres; RT_ERR_ARG for null
   frame pointers, NULL prev_spheres with n_prev > 0, an empty or oversized frame, other flags, or
   out_feat overlapping anything but exactly cur_feat. */
int rt_warp_features_spheres(rt_ctx *ctx, const float *cur_feat, const rt_sphere *prev_spheres, uint32_t n_prev,
                             float *out_feat, uint32_t width, uint32_t height, int flags);
int rt_warp_features_spheres_async(rt_ctx *ctx, const float *cur_feat, const rt_sphere *prev_spheres, uint32_t n_prev,
                                   float *out_feat, uint32_t width, uint32_t height, int flags, void *hip_stream);
/* Device time of the last sphere warp kernel (HIP events of its own), ms; RT_ERR_STATE before a first run. */
int rt_last_sphere_warp_ms(const rt_ctx *ctx, float *ms);

/* ---- variance-guided display filter driven by temporal luminance moments.  The
   rules of the calls above hold: display only, no render state is changed, the accumulation buffer
   is only read, `flags` takes RT_OUT_DEVICE only, the same stream ordering, and arithmetic that a
   float32 restatement reproduces to the bit.  lum(c) = (0.2126f c.x + 0.7152f c.y) + 0.0722f c.z.
   A moments frame is an RGBA32F frame holding (mean of lum, mean of lum^2, 0, 0) over the per-frame
   images of a view.  It is carried across views by rt_reproject and rt_temporal_merge exactly as
   the displayed colour is (same prev_len, features and cameras: the taps, the weights and the
   out_len are the colour's); the caller drops it on a reshape or a scene change. ---- */
typedef struct rt_denoise_var_params {
    uint32_t iterations; /* 1..8 */
    float sigma_lum;     /* luminance tolerance in standard deviations; +INFINITY: the term is off */
    float sigma_normal, sigma_plane; /* as rt_denoise_params */
    float min_len;       /* history length from which the temporal variance estimate is used, >= 2 */
} rt_denoise_var_params;
int rt_denoise_var_defaults(rt_denoise_var_params *p); /* 5, 4.0f, 0.3f, 0.1f, 4.0f */
/* After every progressive frame: cur_rgba is the accumulation buffer after the frame, prev_rgba a
   copy of it taken before the frame, n_cur = max(progression, 1).  The frame's own sample is
   recovered per component as s = prev + (cur - prev) n_cur, negative results to 0; L = lum(s);
   mom_out.x = m.x + (L - m.x) f, mom_out.y = m.y + (L L - m.y) f with f = 1.0f / n_cur, mom_out.zw = 0.
   n_cur == 1: s = cur (negative components to 0), mom_out = (L, L L, 0, 0); prev_rgba and mom_in
   are not read and may be NULL.  mom_out == mom_in is allowed; mom_out may not be prev_rgba or
   cur_rgba, n_cur < 1 or NaN: RT_ERR_ARG. */
int rt_moments_accumulate(rt_ctx *ctx, const float *prev_rgba, const float *cur_rgba, float n_cur, const float *mom_in,
                          float *mom_out, uint32_t width, uint32_t height, int flags);
int rt_moments_accumulate_async(rt_ctx *ctx, const float *prev_rgba, const float *cur_rgba, float n_cur,
                                const float *mom_in, float *mom_out, uint32_t width, uint32_t height, int flags,
                                void *hip_stream);
/* The variance of the displayed (mean) luminance, out_var: one plane of W*H floats.  Per pixel with
   l = len[p] (the history length of the moments and of disp_rgba, the frame about to be displayed):
   l >= min_len: max(m.y - m.x m.x, 0) / (l - 1).  Otherwise a spatial estimate: the 7x7 window at
   unit distance, tap weights exp(-(|dN|^2/sn^2 + (dP.N)^2/sp^2)) as rt_denoise's feature terms,
   d = max(sum(w L_q^2)/sum(w) - (sum(w L_q)/sum(w))^2, 0), out = d (min_len / max(l, 1)).
   Reads sigma_normal, sigma_plane (<= 0 or NaN: RT_ERR_ARG) and min_len (< 2 or NaN: RT_ERR_ARG) of
   `params`.  out_var apart from every input. */
int rt_variance(rt_ctx *ctx, const float *disp_rgba, const float *mom_rgba, const float *len, const float *feat,
                float *out_var, uint32_t width, uint32_t height, const rt_denoise_var_params *params, int flags);
int rt_variance_async(rt_ctx *ctx, const float *disp_rgba, const float *mom_rgba, const float *len, const float *feat,
                      float *out_var, uint32_t width, uint32_t height, const rt_denoise_var_params *params, int flags,
                      void *hip_stream);
/* rt_denoise's filter with its colour term replaced by |lum(c_q) - lum(c_p)| / (sigma_lum sqrt(g) +
   1e-8), g the 3x3 Gaussian of the variance plane around p; the variance is filtered along with the
   colour by the squared weights and feeds the next pass.  in_var: W*H floats >= 0.  out_rgba ==
   in_rgba and out_var == in_var are allowed (no other overlap); out_var may be NULL.  Reads
   iterations (outside 1..8: RT_ERR_ARG) and the three sigmas (<= 0 or NaN: RT_ERR_ARG) of `params`. */
int rt_denoise_var(rt_ctx *ctx, const float *in_rgba, const float *in_var, const float *feat, float *out_rgba,
                   float *out_var, uint32_t width, uint32_t height, const rt_denoise_var_params *params, int flags);
int rt_denoise_var_async(rt_ctx *ctx, const float *in_rgba, const float *in_var, const float *feat, float *out_rgba,
                         float *out_var, uint32_t width, uint32_t height, const rt_denoise_var_params *params, int flags,
                         void *hip_stream);
/* Device time of the last moments kernel, the last variance kernel and all passes of the last
   rt_denoise_var (HIP events of their own), ms; any pointer may be NULL (not all).  RT_ERR_STATE when
   a kernel asked for has not run. */
int rt_last_variance_ms(const rt_ctx *ctx, float *moments_ms, float *variance_ms, float *denoise_var_ms);

/* ---- tone-mapped 8-bit display output with histogram auto-exposure: the last
   display stage, from the shown RGBA32F frame to RGBA8 (GL_RGBA / GL_UNSIGNED_BYTE in memory: the
   word r | g << 8 | b << 16 | 255 << 24, rows in the input's order).  The rules of the calls above
   hold: display only, no render state is changed, the frame is only read, the same stream ordering,
   and arithmetic that a float32 restatement reproduces to the bit (no contraction, IEEE division,
   rt_math.h's rt_powf, rt_minf, rt_maxf; lum as above).  `flags` takes RT_OUT_DEVICE only: with it
   every buffer of a call is a device pointer, the one-float exposure included; without it every
   buffer is host memory and the library stages them.  No input is written. ---- */
enum { RT_TONE_CLAMP = 0, RT_TONE_REINHARD = 1, RT_TONE_ACES = 2 };
enum { RT_METER_BINS = 384 };
typedef struct rt_tonemap_params {
    uint32_t curve;  /* RT_TONE_* */
    uint32_t srgb;   /* non-zero: the sRGB transfer function before the quantisation */
    uint32_t dither; /* non-zero: the 8x8 ordered dither */
    float exposure;  /* the factor on the radiance, when the call is given no metered exposure; > 0 */
    float white;     /* RT_TONE_REINHARD: the luminance that maps to 1; > 0 */
} rt_tonemap_params;
typedef struct rt_meter_params {
    float key;          /* the value the metered mean luminance is brought to; > 0 */
    float lo, hi;       /* the percentile range of the counted pixels that is metered: 0 <= lo < hi <= 1 */
    float e_min, e_max; /* the exposure's bounds: 0 < e_min <= e_max */
    float rate;         /* the share of the way from the previous exposure to the target, in (0, 1] */
} rt_meter_params;
int rt_tonemap_defaults(rt_tonemap_params *p); /* RT_TONE_ACES, 1, 1, 1.0f, 4.0f */
int rt_meter_defaults(rt_meter_params *p);     /* 0.18f, 0.10f, 0.95f, 2^-8, 2^12, 1.0f */
/* The meter.  Histogram, integers only: per pixel L = lum(rgb), u = L's bits; the pixel is counted
   when 0 < u < 0x7f800000 (L positive and finite; zero, negative, NaN, +INFINITY are not), into bin
   min(max((int)(u >> 19) - 1776, 0), 383): exponent and top four mantissa bits, 16 bins per octave
   over 24 octaves from 2^-16 (1776 = bits(2^-16) >> 19).  hist_out: NULL, or RT_METER_BINS counts.
   Exposure, from the counts n_i in index order: N = sum n_i; N == 0: E = prev > 0 ? prev : 1.0f.
   Else lo_n = min((uint64)((double)lo (double)N), N - 1), hi_n = min(max((uint64)((double)hi
   (double)N), lo_n + 1), N); with c_i the count before bin i, k_i the length of [c_i, c_i + n_i) cut
   with [lo_n, hi_n): S = sum k_i (2 i + 1), K = hi_n - lo_n (uint64),
   m = (float)((double)S / (double)(32 K)) - 16.0f (the mean log2 luminance of the range at bin
   centres), Et = rt_minf(rt_maxf(key rt_powf(2.0f, -m), e_min), e_max); E = Et when !(prev > 0) or
   prev is not finite, else prev + (Et - prev) rate.  *exposure_io is read as prev and written as E.
   Null rgba, exposure_io or params, an empty frame, key <= 0 or NaN, lo outside [0, 1), hi outside
   (lo, 1], e_min <= 0 or NaN or above e_max, rate outside (0, 1]: RT_ERR_ARG. */
int rt_meter_exposure(rt_ctx *ctx, const float *rgba, float *exposure_io, uint32_t *hist_out, uint32_t width,
                      uint32_t height, const rt_meter_params *params, int flags);
int rt_meter_exposure_async(rt_ctx *ctx, const float *rgba, float *exposure_io, uint32_t *hist_out, uint32_t width,
                            uint32_t height, const rt_meter_params *params, int flags, void *hip_stream);
/* The tone map, per component c of pixel (x, y) with E = *exposure, or params->exposure when
   `exposure` is NULL: v = c E; v = v > 0 ? v : 0 (NaN too); v = rt_minf(v, 65536.0f).  The curve:
   RT_TONE_CLAMP nothing; RT_TONE_REINHARD L = lum(v), s = (1.0f + L iw) / (1.0f + L) with iw = 1.0f /
   (white white) computed by the host in float, v = v s; RT_TONE_ACES v = (v (2.51f v + 0.03f)) /
   (v (2.43f v + 0.59f) + 0.14f), every operation rounded on its own.  Then v = rt_minf(rt_maxf(v, 0),
   1); with srgb v = v <= 0.0031308f ? 12.92f v : 1.055f rt_powf(v, 0.41666666f) - 0.055f and the same
   clamp again; q = min((int)(v 255.0f + d), 255) with d = 0.5f, or with dither d = ((float)B + 0.5f)
   0.015625f, B the 8x8 Bayer index of (x & 7, y & 7): with a = x ^ y, b = y and bit 0 the least
   significant, B = a0 << 5 | b0 << 4 | a1 << 3 | b1 << 2 | a2 << 1 | b2.  out_rgba8: W*H words.
   Null rgba, out_rgba8 or params, an empty frame, curve beyond RT_TONE_ACES, white <= 0 or NaN,
   params->exposure <= 0 or NaN when it is used: RT_ERR_ARG. */
int rt_tonemap(rt_ctx *ctx, const float *rgba, const float *exposure, uint32_t *out_rgba8, uint32_t width,
               uint32_t height, const rt_tonemap_params *params, int flags);
int rt_tonemap_async(rt_ctx *ctx, const float *rgba, const float *exposure, uint32_t *out_rgba8, uint32_t width,
                     uint32_t height, const rt_tonemap_params *params, int flags, void *hip_stream);
/* Device time of the last meter (the histogram's reset, both kernels) and of the last tone-map kernel
   (HIP events of their own), ms; either pointer may be NULL (not both).  RT_ERR_STATE when a stage
   asked for has not run. */
int rt_last_tonemap_ms(const rt_ctx *ctx, float *meter_ms, float *tonemap_ms);

/* ---- the noise meter: how good is the frame on screen?  The variance plane of a
   frame's luminance (rt_variance's output, or rt_denoise_var's out_var) reduced to a histogram of the
   relative standard error, a per-tile map and one figure a host can act on.  The rules of the calls
   above hold: display only, no render state is changed, both inputs are only read, the same stream
   ordering, arithmetic that a float32 restatement reproduces to the bit (no contraction, IEEE division
   and square root, rt_math.h's rt_maxf; lum as above).  `flags` takes RT_OUT_DEVICE only: with it every
   buffer of a call is a device pointer, stats_out included (the figure then stays on the device, as the
   meter's exposure does); without it every buffer is host memory and the library stages them. ---- */
typedef struct rt_noise_params {
    float percentile; /* the share of the counted pixels whose error the level bounds, in (0, 1] */
    float threshold;  /* the relative error `below` counts against; >= 0 */
    float lum_floor;  /* added to the luminance under the error, so that black pixels count; > 0, finite */
} rt_noise_params;
typedef struct rt_noise_stats {
    float level;      /* an upper bound of the percentile's relative error: its bin's upper edge */
    uint32_t counted; /* the valid pixels */
    uint32_t skipped; /* width height - counted */
    uint32_t below;   /* the pixels in bins whose upper edge is <= threshold */
} rt_noise_stats;
int rt_noise_defaults(rt_noise_params *p); /* 0.95f, 0.05f, 1e-3f */
/* Per pixel p: L = lum(rgba_p), v = var_p.  The pixel is valid when v >= 0, v is finite and L is
   finite; any other is skipped and joins no bin and no tile figure.  For a valid pixel Lp = L > 0 ? L
   : 0, e = rt_sqrtf(v) / (Lp + lum_floor) (one square root, one add, one division), u = bits(e) &
   0x7fffffff, bin min(max((int)(u >> 19) - 1776, 0), 383): rt_meter_exposure's RT_METER_BINS bins, so
   e = 0 is in bin 0 and anything from 2^8 upward in bin 383.  hist_out: NULL, or RT_METER_BINS counts.
   tiles_out: NULL, or ceil(width / 8) x ceil(height / 8) pairs (mean, max), row-major, one for each
   8x8 tile: with j = (y & 7) 8 + (x & 7) and a_j = e for a valid pixel inside the frame, else 0.0f,
   the sum is lane 0's after the butterfly a_j = a_j + a_(j ^ (1 << k)), k = 0..5, all lanes at once
   (the additions commute: every lane holds the same bits), the maximum lane 0's after the same
   butterfly with a_j = rt_maxf(a_j, a_(j ^ (1 << k))); mean = sum / (float)n_valid, one division, and
   with n_valid == 0 both are 0.0f.
   The statistic, from the counts n_i in index order: N = sum n_i (uint64), counted = N, skipped =
   width height - N.  N == 0: level = 0.0f, below = 0.  Else r = min((uint64)((double)percentile
   (double)N), N - 1), i the first bin whose running count exceeds r, level = that bin's upper edge
   u2f((i + 1777) << 19), +INFINITY for bin 383; below = the sum of n_i over the bins whose upper edge
   is <= threshold.  The level is at most 17/16 of the true percentile where that lies in [2^-16, 2^8).
   Null rgba, var, stats_out or params, an empty frame, percentile outside (0, 1], threshold negative
   or NaN, lum_floor not positive and finite, an output overlapping an input or another output:
   RT_ERR_ARG. */
int rt_noise_meter(rt_ctx *ctx, const float *rgba, const float *var, rt_noise_stats *stats_out, float *tiles_out,
                   uint32_t *hist_out, uint32_t width, uint32_t height, const rt_noise_params *params, int flags);
int rt_noise_meter_async(rt_ctx *ctx, const float *rgba, const float *var, rt_noise_stats *stats_out, float *tiles_out,
                         uint32_t *hist_out, uint32_t width, uint32_t height, const rt_noise_params *params, int flags,
                         void *hip_stream);
/* Device time of the last noise meter (the histogram's reset, both kernels; HIP events of its own), ms.
   RT_ERR_STATE when it has not run. */
int rt_last_noise_ms(const rt_ctx *ctx, float *ms);

/* ---- adaptive sampling: stop tracing the tiles the noise meter calls quiet.  A stop
   plane holds one word per 8x8 tile of a frame, ceil(width / 8) x ceil(height / 8) words, row-major, the
   tiles rt_noise_meter's tiles_out is on: 0 = the tile is refined, k > 0 = it stopped after k frames.
   Triangle kernel only (the sphere kernels' seed rows shift with the progression), whole frames only. ---- */
/* Sets the plane that masks the context's renders (stop == NULL: clears it; width, height and flags are
   then not read).  A host pointer is copied at the call (after the renders in flight).  With
   RT_OUT_DEVICE the pointer is borrowed: it is read on each render's stream, so the caller may change
   its contents between renders (ordered against them by the caller), and must keep it alive until it is
   cleared or replaced.  While a plane is set, rt_render / rt_render_async of RT_KERNEL_TRIS with tile ==
   NULL and the plane's width x height renders only the tiles whose word is 0: every pixel of such a tile
   gets exactly the framebuffer value and seed words the unmasked render would have given it, every pixel
   of any other tile keeps its framebuffer value and both seed words.  Such a render is always a
   whole-pixel launch (no sample split, no pilot render), records no pixel costs, and its counters count
   the live tiles' rays.  Any other render while a plane is set — another kernel, a tile, another size —
   is RT_ERR_ARG, never a silent full render.  The display-side calls are not affected.  RT_ERR_ARG for
   an empty or oversized frame and for flags other than RT_OUT_DEVICE. */
int rt_set_tile_stop(rt_ctx *ctx, const uint32_t *stop, uint32_t width, uint32_t height, int flags);
typedef struct rt_adaptive_params {
    float threshold;     /* a tile's mean relative error at or under which it is quiet; >= 0 */
    float max_ratio;     /* ... with its maximum at or under threshold max_ratio; >= 1, +INFINITY: the term is off */
    uint32_t min_frames; /* no tile is quiet before the view has this many frames */
    uint32_t dilate;     /* a tile stops only when every tile within this many tiles of it is settled; 0..4 */
} rt_adaptive_params;
typedef struct rt_adaptive_stats {
    uint32_t tiles;       /* the tile count */
    uint32_t active;      /* the live tiles after the call */
    uint32_t stopped_now; /* the tiles this call stopped */
    uint32_t frames;      /* n_frames */
} rt_adaptive_stats;
int rt_adaptive_defaults(rt_adaptive_params *p); /* 0.05f, 4.0f, 16, 1 */
/* The stop rule.  tiles_mean_max: rt_noise_meter's tiles_out, pairs (mean, max).  Tile t is quiet when
   n_frames >= min_frames, mean <= threshold and max <= lim, with lim the float product threshold
   max_ratio formed by the host, or +INFINITY when max_ratio is (a NaN of the map is under neither; a
   tile with no valid pixel reads (0, 0) and is quiet).  It is settled when stop_io[t] != 0 or it is
   quiet.  A live tile (stop_io[t] == 0) is stopped, stop_io[t] = n_frames, exactly when every tile
   inside the frame within `dilate` tiles of it (Chebyshev distance, itself included) is settled; every
   tile is decided from the plane as it was before the call.  A stopped tile's word is never changed:
   stopping is monotone.  Only comparisons and integers: the result is exact.  The rules of the display
   stages hold: no render state is changed, `flags` takes RT_OUT_DEVICE only (with it every buffer is a
   device pointer, stats_out included), the same stream ordering — a render enqueued after the call
   sees the new plane.  Null pointers, an empty frame, n_frames == 0, threshold negative or NaN,
   max_ratio < 1 or NaN, dilate > 4, overlapping buffers: RT_ERR_ARG. */
int rt_tile_stop_select(rt_ctx *ctx, const float *tiles_mean_max, uint32_t *stop_io, uint32_t n_frames,
                        rt_adaptive_stats *stats_out, uint32_t width, uint32_t height, const rt_adaptive_params *params,
                        int flags);
int rt_tile_stop_select_async(rt_ctx *ctx, const float *tiles_mean_max, uint32_t *stop_io, uint32_t n_frames,
                              rt_adaptive_stats *stats_out, uint32_t width, uint32_t height,
                              const rt_adaptive_params *params, int flags, void *hip_stream);
/* The pixel queue's order under a plane, as a masked render computes it before its launch: order_out
   (n_tiles words) receives the entries of `base` (a tile order of n_tiles words; NULL: 0, 1, ...) whose
   tile's word of `stop` (n_tiles words) is 0, in base's order, then n_tiles — the first index outside
   the frame, which the kernel's queue rejects — in every remaining position; *live_out their number.
   An entry of base that is no tile index counts as stopped.  The display stages' rules as above.  Null
   stop or outputs, n_tiles 0 or above 2^28 - 1, an output overlapping an input or the other output:
   RT_ERR_ARG. */
int rt_tile_stop_order(rt_ctx *ctx, const uint32_t *base, const uint32_t *stop, uint32_t n_tiles, uint32_t *order_out,
                       uint32_t *live_out, int flags);
int rt_tile_stop_order_async(rt_ctx *ctx, const uint32_t *base, const uint32_t *stop, uint32_t n_tiles,
                             uint32_t *order_out, uint32_t *live_out, int flags, void *hip_stream);
/* rt_moments_accumulate under a plane, with the history lengths rt_variance needs.  A pixel of a live
   tile (stop[t] == 0): exactly rt_moments_accumulate, and len_out[p] = n_cur.  A pixel of a stopped
   tile was not traced (cur == prev there: the recovered "sample" would be its own mean): mom_out =
   mom_in, and len_out[p] = (float)stop[t].  mom_in may be NULL only with n_cur == 1; a stopped tile's
   mom_out is then left as it is.  len_out: W*H floats apart from every other buffer; the plane apart
   from mom_out; otherwise rt_moments_accumulate's rules and errors. */
int rt_moments_accumulate_tiles(rt_ctx *ctx, const float *prev_rgba, const float *cur_rgba, float n_cur,
                                const float *mom_in, float *mom_out, const uint32_t *stop, float *len_out, uint32_t width,
                                uint32_t height, int flags);
int rt_moments_accumulate_tiles_async(rt_ctx *ctx, const float *prev_rgba, const float *cur_rgba, float n_cur,
                                      const float *mom_in, float *mom_out, const uint32_t *stop, float *len_out,
                                      uint32_t width, uint32_t height, int flags, void *hip_stream);
/* Device time of the last stop rule (the stats' reset, both kernels) and of the last masked order kernel
   (a masked render's, or rt_tile_stop_order's; HIP events of their own), ms; either pointer may be NULL
   (not both).  RT_ERR_STATE when a stage asked for has not run.  rt_moments_accumulate_tiles' time is
   rt_last_variance_ms' moments_ms. */
int rt_last_adaptive_ms(const rt_ctx *ctx, float *select_ms, float *order_ms);

/* ---- per-tile sample counts: extra passes per display for the noisy tiles.  The planes
   hold one word per 8x8 tile, as a stop plane does.  A tile is traced by a masked render at progression
   0 into a scratch frame — which overwrites the live tiles' pixels with the frame's own sample — and
   folded into the accumulation buffer afterwards with the weight its own count gives: the triangle
   kernel needs no per-tile weight. ---- */
#define RT_BUDGET_MAX_PASSES 8
/* The fold.  Tile t is folded when passes == NULL or passes[t] > pass.  A folded tile: c = count_io[t], p =
   c + 1 saturating at 2^32 - 1, n = (float)p, w = 1.0f / n; every pixel of the tile inside the frame gets
   acc = old + (sample - old) w on all four channels (subtract, multiply, add: the progressive render's own
   mix, at p == 1 too), with the moments given mom_out = rt_moments_accumulate's moments after a frame with
   prev = old, cur = new, n_cur = n (its n == 1 branch included), and len_out = n; then count_io[t] = p.  A
   tile that is not folded keeps acc and its count; mom_out gets mom_in where the two are different
   buffers, and len_out = (float)count_io[t].  sample_rgba is only read.  mom_in and mom_out are both given
   or both NULL and may be the same buffer; len_out may be NULL; nothing else may overlap anything
   (RT_ERR_ARG).  This is the first display-side entry that writes an accumulation buffer; it still touches
   no render state — seeds, schedule, lists, counters, rt_last_*.  Otherwise the display stages' rules, as
   rt_moments_accumulate_tiles: `flags` takes RT_OUT_DEVICE only, host arrays are staged, the same stream
   ordering.  Null sample, acc or count, an empty or oversized frame: RT_ERR_ARG. */
int rt_fold_tiles(rt_ctx *ctx, const float *sample_rgba, float *acc_rgba, uint32_t *count_io, const uint32_t *passes,
                  uint32_t pass, const float *mom_in, float *mom_out, float *len_out, uint32_t width, uint32_t height,
                  int flags);
int rt_fold_tiles_async(rt_ctx *ctx, const float *sample_rgba, float *acc_rgba, uint32_t *count_io, const uint32_t *passes,
                        uint32_t pass, const float *mom_in, float *mom_out, float *len_out, uint32_t width, uint32_t height,
                        int flags, void *hip_stream);
typedef struct rt_budget_params {
    uint32_t max_passes;                     /* the most passes a tile gets in one display; 1..RT_BUDGET_MAX_PASSES */
    float limits[RT_BUDGET_MAX_PASSES - 1]; /* the first max_passes - 1 are read: >= 0, strictly ascending, no NaN */
} rt_budget_params;
typedef struct rt_budget_stats {
    uint32_t tiles;       /* the tile count */
    uint32_t rounds;      /* the largest pass count a tile got */
    uint32_t tile_passes; /* the sum of the pass counts */
    uint32_t reserved;    /* 0 */
    uint32_t by_passes[RT_BUDGET_MAX_PASSES + 1]; /* [i]: the tiles with i passes */
} rt_budget_stats;
int rt_budget_defaults(rt_budget_params *p); /* 4, {0.1f, 0.2f, 0.4f, ...}: the meter's threshold x 2, 4, 8 */
/* The budget rule on rt_noise_meter's tile map: passes_out[t] = 0 where stop[t] != 0 (stop may be NULL: no
   tile is stopped), elsewhere 1 + the number of k < max_passes - 1 with mean_t > limits[k].  Comparisons
   only: a NaN mean is above nothing and gives 1, as does a tile with no valid pixel, which reads (0, 0).
   The relative error falls as 1 / sqrt(n), so a tile at twice a limit needs four times its samples: the
   defaults are a coarse monotone step towards that, and the table is the caller's policy.  The display
   stages' rules as above.  Null map, output or stats, max_passes outside 1..8, a limit read that is NaN,
   negative or not above the one before it, overlapping buffers: RT_ERR_ARG. */
int rt_tile_budget(rt_ctx *ctx, const float *tiles_mean_max, const uint32_t *stop, uint32_t *passes_out,
                   rt_budget_stats *stats_out, uint32_t width, uint32_t height, const rt_budget_params *params, int flags);
int rt_tile_budget_async(rt_ctx *ctx, const float *tiles_mean_max, const uint32_t *stop, uint32_t *passes_out,
                         rt_budget_stats *stats_out, uint32_t width, uint32_t height, const rt_budget_params *params,
                         int flags, void *hip_stream);
/* The plane of pass `pass`, in rt_set_tile_stop's sense: mask_out[t] = 0 (rendered) where stop[t] == 0 (or
   stop is NULL) and passes[t] > pass, else 1.  The display stages' rules; mask_out apart from both inputs. */
int rt_tile_pass_mask(rt_ctx *ctx, const uint32_t *stop, const uint32_t *passes, uint32_t pass, uint32_t *mask_out,
                      uint32_t width, uint32_t height, int flags);
int rt_tile_pass_mask_async(rt_ctx *ctx, const uint32_t *stop, const uint32_t *passes, uint32_t pass, uint32_t *mask_out,
                            uint32_t width, uint32_t height, int flags, void *hip_stream);
/* Device time of the last fold, budget rule (its stats' reset included) and pass mask, ms; any pointer may be
   NULL (not all).  RT_ERR_STATE when a stage asked for has not run. */
int rt_last_budget_ms(const rt_ctx *ctx, float *fold_ms, float *budget_ms, float *mask_ms);

/* ---- adaptive sampling under the temporal stage: per-pixel frame counts.  Under a stop
   plane or a count plane the accumulation buffer's frame count differs from tile to tile; these are the
   temporal merge and the trust test with that count as a plane (rt_moments_accumulate_tiles' and
   rt_fold_tiles' len_out), the shortest merged history of every tile, and the stop rule gated by it.  The
   rules of their scalar twins hold for all four: display only — no render state is changed —, `flags`
   takes RT_OUT_DEVICE only, host buffers are staged, the same stream ordering, no contraction and IEEE
   division. ---- */
/* rt_temporal_merge with the frame count per pixel: n = cur_len[p] >= 1 ? cur_len[p] : 1.0f (a NaN and a 0
   read as 1: a tile stopped before its first fold has count 0), then that entry's arithmetic with this n —
   where m = hist_len[p] > 0: l = n + m, f = n / l, out = h + (c - h) f on rgb; elsewhere c's bits and l = n;
   out.a = c.a and out_len = l < max_history ? l : max_history in both.  out_rgba == hist_rgba and out_len
   == hist_len are allowed; cur_len (W*H floats) lies apart from both outputs.  out_rgba == cur_rgba, a
   null pointer, an empty frame, max_history < 1 or NaN, cur_len overlapping an output: RT_ERR_ARG.  Its
   device time is rt_last_reproject_ms' merge_ms. */
int rt_temporal_merge_len(rt_ctx *ctx, const float *hist_rgba, const float *hist_len, const float *cur_rgba,
                          const float *cur_len, float max_history, float *out_rgba, float *out_len, uint32_t width,
                          uint32_t height, int flags);
int rt_temporal_merge_len_async(rt_ctx *ctx, const float *hist_rgba, const float *hist_len, const float *cur_rgba,
                                const float *cur_len, float max_history, float *out_rgba, float *out_len, uint32_t width,
                                uint32_t height, int flags, void *hip_stream);
/* rt_history_trust with n_cur replaced, in both places it appears (vh max(m, 1) / n and 1 + n / m), by the
   centre pixel's n (the clamp above).  The window's taps are unchanged: where the 7 x 7 window reaches into
   tiles of other counts their taps are weighed as if they had the centre's — an approximation (DESIGN.md
   §8).  tolerance = +INFINITY returns hist_len bit for bit.  out_len == hist_len is allowed, cur_len lies
   apart from out_len; otherwise rt_history_trust's rules and errors.  Its device time is rt_last_trust_ms. */
int rt_history_trust_len(rt_ctx *ctx, const float *hist_rgba, const float *hist_len, const float *cur_rgba,
                         const float *cur_len, const float *feat, float *out_len, uint32_t width, uint32_t height,
                         const rt_trust_params *params, int flags);
int rt_history_trust_len_async(rt_ctx *ctx, const float *hist_rgba, const float *hist_len, const float *cur_rgba,
                               const float *cur_len, const float *feat, float *out_len, uint32_t width, uint32_t height,
                               const rt_trust_params *params, int flags, void *hip_stream);
/* One float per 8x8 tile on the noise meter's tile grid (ceil(width / 8) x ceil(height / 8), row-major):
   the minimum of v = len[p] > 0 ? len[p] : 0.0f (a negative length, a NaN and -0 read as +0) over the
   tile's pixels inside the frame — with feat (the two feature planes; NULL: every pixel counts) over
   those that met a surface (id != RT_FEAT_NONE): a background pixel never gets a history and must not keep
   its tile alive.  A tile with no counted pixel reads +INFINITY.  A minimum is exact in any order.  tiles_out
   apart from both inputs.  Null len or tiles_out, an empty frame, an overlap: RT_ERR_ARG. */
int rt_tile_len_min(rt_ctx *ctx, const float *len, const float *feat, float *tiles_out, uint32_t width, uint32_t height,
                    int flags);
int rt_tile_len_min_async(rt_ctx *ctx, const float *len, const float *feat, float *tiles_out, uint32_t width,
                          uint32_t height, int flags, void *hip_stream);
/* Device time of the last rt_tile_len_min, ms.  RT_ERR_STATE when it has not run. */
int rt_last_tile_len_ms(const rt_ctx *ctx, float *ms);
/* rt_tile_stop_select with the frame gate per tile: tile t can be quiet only when tile_frames[t] >=
   (float)min_frames (a NaN does not pass), where the scalar form asks n_frames >= min_frames.  Everything
   else is that entry's: the dilation, monotone stopping, stop_io[t] = n_frames for a tile stopped now — the
   stop word remains the accumulation buffer's own frame count, which rt_moments_accumulate_tiles reads as
   such —, the stats, the errors.  tile_frames (a float per tile) is only read and lies apart from stop_io
   and stats_out.  Its device time is rt_last_adaptive_ms' select_ms. */
int rt_tile_stop_select_frames(rt_ctx *ctx, const float *tiles_mean_max, const float *tile_frames, uint32_t *stop_io,
                               uint32_t n_frames, rt_adaptive_stats *stats_out, uint32_t width, uint32_t height,
                               const rt_adaptive_params *params, int flags);
int rt_tile_stop_select_frames_async(rt_ctx *ctx, const float *tiles_mean_max, const float *tile_frames, uint32_t *stop_io,
                                     uint32_t n_frames, rt_adaptive_stats *stats_out, uint32_t width, uint32_t height,
                                     const rt_adaptive_params *params, int flags, void *hip_stream);

/* ---- synthetic meshes (deterministic, host-independent: rt_math.h only) ----
   A displaced lat-long sphere truncated to exactly n_tris triangles, centred at
   (cx, cy, cz) with base radius r.  verts must hold rt_mesh_vertex_count(n_tris)
   xyz triples, idx 3*n_tris ints. */
uint32_t rt_mesh_vertex_count(uint32_t n_tris);
int rt_make_mesh(uint32_t n_tris, float cx, float cy, float cz, float r, float *verts_xyz, int32_t *idx);

/* ---- PLY meshes: PLYLoader (clrt/PLYLoader.cpp:4-90) over ply.c (ply.c:2457-2720).
   ascii / binary_little_endian / binary_big_endian; vertex x, y, z as float32, face
   `vertex_indices` lists (polygons fan-triangulated, < 3 vertices dropped, indices
   range-checked — the reference copies only 2-vertex faces, PLYLoader.cpp:74); other
   properties and elements skipped.  open decodes the file and reports the counts;
   read copies into caller buffers (3*n_verts floats, 3*n_tris ints). ---- */
typedef struct rt_ply rt_ply;
int rt_ply_open(const char *path, rt_ply **out, uint32_t *n_verts, uint32_t *n_tris);
int rt_ply_read(const rt_ply *ply, float *verts_xyz, int32_t *idx);
uint32_t rt_ply_dropped_faces(const rt_ply *ply);
int rt_ply_close(rt_ply *ply);
const char *rt_ply_last_error(void); /* message of the last failed rt_ply_open (this thread's process) */
/* Scale uniformly to `max_extent` on the longest axis, centre x and z on 0 and rest the
   lowest point on y = floor_y (extent 3 on the box floor y = -5). */
int rt_normalize_mesh(float *verts_xyz, uint32_t n_verts, float max_extent, float floor_y);

/* ---- multi-GPU from the native host: one process (or thread) per GPU, RCCL over
   xGMI.  The reference renders on one OpenCL device (RayTracerCL.cpp:52-145,
   :217-307); this is the sharded form of the same rayTrace call, with no data-path
   exchange (pixels are independent) besides the frame assembly, plus the seed-row
   halo of progressive sphere frames.  A communicator is created collectively:
   rank 0 makes the id, the caller hands the bytes to every rank by any channel
   (MPI, a file, a TCP store), each rank calls rt_comm_create with its own GPU. ---- */
typedef struct rt_comm rt_comm;
#define RT_COMM_ID_BYTES 128
/* ncclGetUniqueId (rccl.h:187). */
int rt_comm_get_unique_id(uint8_t id[RT_COMM_ID_BYTES]);
/* ncclCommInitRank (rccl.h:215) on `device`; collective over n_ranks callers. */
int rt_comm_create(const uint8_t id[RT_COMM_ID_BYTES], int n_ranks, int rank, int device, rt_comm **out);
int rt_comm_destroy(rt_comm *comm);
const char *rt_comm_last_error(const rt_comm *comm);
/* ncclCommCount (rccl.h:378): ranks in the communicator as RCCL sees them. */
int rt_comm_count(const rt_comm *comm, int *n_ranks);
/* Frame assembly (collective): every rank passes its compact tile (device pointer,
   rt_tile_rows(H, {stripe, n_ranks, rank, stripe_owner}) rows of W RGBA32F pixels); `root`
   receives them with grouped ncclSend/ncclRecv (one point-to-point xGMI transfer per sender)
   and scatters the stripes into `frame_dev` (device, W*H*4 floats; others: ignored).
   stripe_owner: the partition the tiles were rendered with (NULL: interleaved). */
int rt_comm_gather_frame(rt_comm *comm, const float *tile_dev, float *frame_dev, uint32_t width, uint32_t height,
                         uint32_t stripe_rows, const uint32_t *stripe_owner, int root);
/* Device-side assembly on one GPU: n_ranks compact tiles (device pointers, rank
   order) scattered into frame_dev (the root's step of rt_comm_gather_frame). */
int rt_assemble_tiles(const float *const *tiles_dev, uint32_t n_ranks, uint32_t width, uint32_t height,
                      uint32_t stripe_rows, const uint32_t *stripe_owner, float *frame_dev, int device);
/* Seed-row halo plan (host only).  writer[Hpad]: last rank that wrote each seed row
   (-1: nobody, the initial seeds are identical on every rank).  Before a raytrace
   frame with row shift `progressive` under the partition (stripe_rows, n_ranks,
   stripe_owner: NULL = interleaved), lists the moves (src rank, dst rank, seed row) that
   bring every row a rank reads up to date — including rows whose stripe changed owner since
   it was written; then records the frame's writes in writer.  Capacity of the three output
   arrays: height entries. */
int rt_seed_halo_plan(int32_t *writer, uint32_t height, uint32_t hpad, uint32_t stripe_rows, uint32_t n_ranks,
                      const uint32_t *stripe_owner, uint32_t progressive, uint32_t *src, uint32_t *dst,
                      uint32_t *rows, uint32_t *n_moves);
/* One rank's side of a halo plan (host only): the rows `me` sends to each peer and receives
   from each peer, as one packed block per peer in peer order — send_rows holds the blocks to
   peers 0, 1, ... back to back (send_counts[p] rows to peer p), likewise recv_rows /
   recv_counts.  Row order within a block is the plan's, so peer p's send block to `me` and
   my receive block from p list the same rows in the same order (the packed buffers match
   word for word).  Capacity of send_rows / recv_rows: n_moves; of the counts: n_ranks. */
int rt_seed_halo_peer_blocks(const uint32_t *src, const uint32_t *dst, const uint32_t *rows, uint32_t n_moves,
                             uint32_t n_ranks, uint32_t me, uint32_t *send_rows, uint32_t *send_counts,
                             uint32_t *recv_rows, uint32_t *recv_counts);
/* One sharded rayTrace (collective): rank renders its stripes into a tile buffer the
   communicator keeps (progression mixes into it across frames), first brings the seed rows
   it reads up to date from their last writers (the seed-row halo: grouped ncclSend/ncclRecv
   of packed rows; raytrace shifts rows by the progression, the other kernels read row y,
   which after progressive sphere frames another rank may have written last), then
   gathers the frame to `root` (frame_dev: device, W*H*4 floats on root).  Bit-identical
   to rt_render of the whole frame on one GPU.  Call rt_comm_reset_halo after replacing
   a context's seeds (rt_set_seeds).  The stripes are dealt by the communicator's partition
   (rt_comm_set_partition). */
int rt_comm_render(rt_comm *comm, rt_ctx *ctx, float *frame_dev, uint32_t width, uint32_t height,
                   uint32_t progression, int kernel, uint32_t stripe_rows, int root);
int rt_comm_reset_halo(rt_comm *comm);
/* Partition of rt_comm_render's frames: RT_PARTITION_INTERLEAVED (stripe s to rank
   s % n_ranks) or RT_PARTITION_BALANCED (the default: raytrace_tris frames by
   rt_partition_stripes, computed by every rank for each new view, every rank then taking the
   root's map from one broadcast; sphere frames stay interleaved).  A change of owner moves the
   stripe's seed rows through the halo (rt_seed_halo_plan).  rt_comm_last_partition copies
   the last frame's owner map (cap entries; *n = its stripes). */
enum { RT_PARTITION_INTERLEAVED = 0, RT_PARTITION_BALANCED = 1 };
int rt_comm_set_partition(rt_comm *comm, int mode);
int rt_comm_last_partition(const rt_comm *comm, uint32_t *owner, uint32_t cap, uint32_t *n);

#ifdef __cplusplus
}
#endif

#endif /* PATHTRACER_RT_H */
