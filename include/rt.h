/*
 * rt.h — C ABI of the MI355X-native path tracer (drop-in for the render path of
 * shaunplee/ray-tracing).
 *
 * The reference has no FFI: its render boundary is the pure Haskell call
 *     runRender :: RenderStaticEnv -> [RandGen] -> [VV.Vector RGB]     (src/Lib.hs:1491)
 * with the environment built by
 *     mkRenderStaticEnv scene camera (w,h) ns maxDepth nThreads        (src/Lib.hs:92-108)
 * and   type Scene = (Hittable world, Hittable lights, Albedo background)  (src/Lib.hs:84).
 * This header replaces that call with plain C: the immutable Haskell `Scene` becomes a
 * flattened `rt_scene_desc` (arrays of POD records), the `Camera` becomes `rt_camera`,
 * `[RandGen]` becomes an array of SplitMix64 (seed, gamma) pairs, and the lazily streamed
 * `[Vector RGB]` becomes a caller-owned H*W*3 byte buffer (top row first, PPM order).
 *
 * Scene construction (Lib.hs constructors, makeBVH, makePerlin, Scenes.hs builders and
 * cameras) is exported too (rt_builder_*, rt_scene_named, rt_camera_*), so a host that
 * used the reference's Scenes.hs API finds the same surface here.
 *
 * Conventions: every function returns 0 on success and a negative RT_E* code on error;
 * the message is available from rt_last_error() (thread-local). No torch / C++ types.
 */
#ifndef RT_H
#define RT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_ABI_VERSION 1

/* ------------------------------------------------------------------ error codes */
#define RT_OK 0
#define RT_E_INVALID (-1)   /* bad argument / malformed scene                       */
#define RT_E_HIP (-2)       /* HIP runtime error                                     */
#define RT_E_NOMEM (-3)     /* allocation failure                                    */
#define RT_E_UNSUPPORTED (-4)/* scene uses a construct the device path does not take */
#define RT_E_STATE (-5)     /* call order (e.g. render before upload)                */
#define RT_E_COMM (-6)      /* RCCL error (multi-device contexts)                    */

/* ------------------------------------------------------------------ scene records */

/* Flattened `Hittable` (src/Lib.hs:521-585). One 64-byte record per constructor. */
enum rt_node_type {
    RT_NODE_BVH = 0,             /* BVHNode left right box size        (Lib.hs:552-560) */
    RT_NODE_SPHERE = 1,          /* Sphere center radius material      (Lib.hs:522-528) */
    RT_NODE_MOVING_SPHERE = 2,   /* MovingSphere c0 c1 t0 t1 dur r mat (Lib.hs:529-543) */
    RT_NODE_RECT_XY = 3,         /* Rect (XYRect x0 x1 y0 y1 k mat)    (Lib.hs:608-620) */
    RT_NODE_RECT_XZ = 4,         /* Rect (XZRect x0 x1 z0 z1 k mat)    (Lib.hs:621-633) */
    RT_NODE_RECT_YZ = 5,         /* Rect (YZRect y0 y1 z0 z1 k mat)    (Lib.hs:634-646) */
    RT_NODE_CUBOID = 6,          /* Cuboid min max [6 rects]           (Lib.hs:545-551,594-605) */
    RT_NODE_TRANSLATE = 7,       /* Translate offset child             (Lib.hs:561-565) */
    RT_NODE_ROTATE = 8,          /* Rotate axis sin cos box child      (Lib.hs:566-576) */
    RT_NODE_CONSTANT_MEDIUM = 9, /* ConstantMedium (-1/density) mat boundary (Lib.hs:577-583) */
    RT_NODE_UNHITTABLE = 10,     /* Unhittable                         (Lib.hs:584) */
    RT_NODE_EXT = 11             /* payload continuation of the previous record (never a child) */
};

/*
 * Field use per type (f = 6 doubles, a/b/c = int32):
 *   BVH            f = box min xyz, box max xyz;   a = left, b = right
 *   SPHERE         f[0..2] = center, f[3] = radius; a = material
 *   MOVING_SPHERE  f[0..2] = center0, f[3..5] = center1; a = material;
 *                  the next record (type EXT) holds f[0]=time0, f[1]=time1, f[2]=duration, f[3]=radius
 *   RECT_XY/XZ/YZ  f[0..4] = (i0, i1, j0, j1, k) in the constructor's argument order; a = material
 *   CUBOID         f = min xyz, max xyz; a = material (the six rects are implied, Lib.hs:599-604)
 *   TRANSLATE      f[0..2] = offset; a = child
 *   ROTATE         f[0] = sin theta, f[1] = cos theta; a = child; b = axis (0 X, 1 Y, 2 Z)
 *   CONSTANT_MEDIUM f[0] = negative inverse density; a = boundary; b = phase material; f[1] = 0, or the
 *                  occurrence key + 1 of an unfolded medium record (rt_rebuild_bvh output; see
 *                  RT_RNG_PHILOX: the upload keys every medium occurrence of the caller's tree)
 * For every type c = htblSize of the node (Lib.hs:662-671): BVH its size, Translate/Rotate
 * the size of the child, Unhittable 0, everything else 1. (World-only BVH nodes appended by the
 * device-side rebuild carry 0x40000000 | split axis instead; they never occur in a lights tree.)
 */
#define RT_BVH_ORDERED 0x40000000 /* rebuilt world BVH node: c = this flag | split axis */
#define RT_BVH_MEDIA_FIRST 0x10000000 /* with RT_BVH_ORDERED: a rebuilt world's top node whose left child
                                         is a medium occurrence (not inside an instance frame), entered
                                         before the right child (the rest of the world) whatever the ray
                                         direction: its candidate bounds the walk from the start */

typedef struct rt_node {
    double f[6];
    int32_t type;
    int32_t a;
    int32_t b;
    int32_t c;
} rt_node; /* 64 bytes */

/* `Material` (src/Lib.hs:339-345). */
enum rt_material_type {
    RT_MAT_LAMBERTIAN = 0,
    RT_MAT_METAL = 1,
    RT_MAT_DIELECTRIC = 2,
    RT_MAT_DIFFUSE_LIGHT = 3,
    RT_MAT_ISOTROPIC = 4
};

typedef struct rt_material {
    int32_t type;
    int32_t texture; /* texture id (Lambertian, Metal, DiffuseLight, Isotropic) */
    double param;    /* Metal: fuzz; Dielectric: refractive index */
} rt_material;       /* 16 bytes */

/* `Texture` (src/Lib.hs:394-419). */
enum rt_texture_type {
    RT_TEX_CONSTANT = 0, /* f[0..2] = albedo */
    RT_TEX_CHECKER = 1,  /* a = odd texture, b = even texture */
    RT_TEX_PERLIN = 2,   /* a = perlin table id, f[0] = scale */
    RT_TEX_IMAGE = 3     /* a = image id (-1 = Nothing), b = width, c = height */
};

typedef struct rt_texture {
    int32_t type;
    int32_t a;
    int32_t b;
    int32_t c;
    double f[4];
} rt_texture; /* 48 bytes */

/* Perlin tables of `makePerlin` (src/Lib.hs:424-439). */
typedef struct rt_perlin {
    double ranvec[256][3];
    int32_t perm_x[256];
    int32_t perm_y[256];
    int32_t perm_z[256];
} rt_perlin; /* 9216 bytes */

/* RGB8 raster (the JuicyPixels `Image PixelRGB8` of src/Lib.hs:384-389), row-major, row 0 = top. */
typedef struct rt_image {
    int64_t offset; /* byte offset into rt_scene_desc.image_pool */
    int32_t width;
    int32_t height;
} rt_image;

typedef struct rt_scene_desc {
    const rt_node* nodes;
    int32_t n_nodes;
    int32_t world_root;  /* node id of the world Hittable */
    int32_t lights_root; /* node id of the lights Hittable; -1 = Unhittable */
    int32_t n_materials;
    const rt_material* materials;
    const rt_texture* textures;
    int32_t n_textures;
    int32_t n_perlins;
    const rt_perlin* perlins;
    const rt_image* images;
    int32_t n_images;
    int32_t _pad;
    const uint8_t* image_pool;
    int64_t image_pool_bytes;
    double background[3]; /* Albedo background (src/Lib.hs:84) */
} rt_scene_desc;

/* `Camera` (src/Lib.hs:1230-1251), as computed by newCamera (src/Lib.hs:1280-1295). */
typedef struct rt_camera {
    double origin[3];
    double llc[3];
    double horiz[3];
    double vert[3];
    double u[3];
    double v[3];
    double w[3];
    double lens_radius;
    double t0;
    double t1;
} rt_camera;

/* ------------------------------------------------------------------ render parameters */

/*
 * RNG stream layouts.
 *  RT_RNG_EXACT  (tier A): the reference's layout — one SplitMix64 generator per image
 *                column, threaded top row to bottom row, through every sample and bounce
 *                (src/Lib.hs:1491-1523, 1352-1371). Only width-parallel.
 *  RT_RNG_PHILOX (tier B): one Philox4x32-10 stream per (pixel, sample), key = seed,
 *                counter = {draw_pair, sample, pixel_id, 0}; each 128-bit block yields two
 *                64-bit words, converted exactly as random-1.2.0 `random :: Double`.
 *                A pixel's samples are summed in fixed chunks: chunk k holds samples
 *                [k*CH, min(spp, (k+1)*CH)) with CH = rt_sample_chunk(width*height, spp);
 *                each chunk is summed in sample order from 0, the chunk sums in chunk order
 *                from 0. (The chunks are the device's work-items; a definition fixed by
 *                (width, height, spp) keeps the image independent of scheduling and shard
 *                count.) Embarrassingly parallel.
 *                A progressive frame opened with RT_FRAME_MOMENTS also keeps, per pixel and channel,
 *                Q = sum over chunks of (S_k * S_k) / (double)n_k in chunk order from 0 (S_k the chunk's
 *                sum, n_k its sample count): the second moment its error estimate rests on, defined
 *                with the frames below.
 *                A tier-B path ends once its throughput is NaN in all three channels (the Lambertian
 *                mixture quirk's 0 / 0, src/Lib.hs:823-836, in a world without lights): background,
 *                emission and depth exhaustion all give throughput * x = (NaN, NaN, NaN) from there,
 *                and the draws the rest of the path would make belong to this sample's stream alone,
 *                so the sample adds throughput * 0 at once. Every sample is still started, counted
 *                and summed in order; the image is the one full paths give (NaNs by mask). Zero
 *                throughput, or one or two NaN channels, end nothing. Tier A traces every path to its
 *                end: a column's stream runs through every draw of every sample.
 *                ConstantMedium (src/Lib.hs:1053-1080) in tier B: its draw is not the stream's next
 *                but the first word of the block at counter {stream words consumed so far, sample,
 *                pixel_id, 2^31 | key}, key = the occurrence's preorder rank among the medium
 *                occurrences of the caller's world tree (BVH left child first, into Translate/Rotate;
 *                one occurrence per path) or f[1] - 1 when set; and its candidate hit is computed over
 *                the boundary's whole inside, then accepted like a leaf's at t <= the bound. The
 *                closest hit is then the least t over every leaf in any walk order (exact ties are
 *                resolved in the reference's order), so media worlds walk re-bounded trees too.
 *                Tier A keeps the reference's own medium: the stream's next draw, under the walk's bound.
 */
#define RT_RNG_EXACT 0
#define RT_RNG_PHILOX 1
#define RT_CHUNK_SAMPLES 8      /* samples per chunk, at least (short chunks: a short tail per shard) */
#define RT_CHUNK_MAX 128         /* ...but at most this many chunks per pixel (bounds the chunk sums) */
#define RT_CHUNK_ITEMS (1 << 20) /* ...fewer samples when the frame would have fewer work-items */
/* CH = min(spp, max(8, ceil(spp / 128)), max(1, ceil(pixels * spp / 2^20))): 8-sample chunks
   (C2, C3/C4 at 1000 spp), longer ones for higher spp (C5 2000 spp: 16) so that a pixel has at most
   128, and shorter ones for small frames (config 1: 200x100x10 -> 1) so that they fill the device.
   (Round 4: 128, was 64 — 16-sample chunks left C4 a long per-shard tail at 8 GPUs.) */
static inline int rt_sample_chunk(int64_t pixels, int spp) {
  const int64_t fill = (pixels * (int64_t)spp + RT_CHUNK_ITEMS - 1) / RT_CHUNK_ITEMS;
  int ch = (spp + RT_CHUNK_MAX - 1) / RT_CHUNK_MAX;
  if (ch < RT_CHUNK_SAMPLES) ch = RT_CHUNK_SAMPLES;
  if (ch > spp) ch = spp;
  if (fill < ch) ch = (int)fill;
  return ch > 0 ? ch : 1;
}

/* Flags. */
#define RT_FLAG_NAN_CULL 1u /* tier B only: stop tracing a pixel once its sum is NaN
                               (its output byte is then fixed at 0, src/Lib.hs:287-288).
                               Output-identical; off by default. */
#define RT_FLAG_REFERENCE_CULL 2u /* cull BVH boxes with the reference's per-axis test only
                               (src/Lib.hs:798-814). Default: that test AND the joint slab test,
                               which prunes only hits that the reference takes by rounding, where the
                               exact ray misses the leaf or touches its rim: a sphere reports hits up to
                               about |o - c|^2 * 2^-52 / r outside itself for a tangent ray, 2^4 radii
                               of a unit sphere from 2^28 away ("Far origins"). A world
                               with a finite BVH box coordinate beyond 2^100 always takes this flag. */
#define RT_FLAG_NAN_ZERO 4u /* tiers A and B, parity diagnostic (NOT the reference's semantics): a sample
                               contribution channel that is NaN is added as 0, so that the finite
                               part of every sample reaches the average. The reference's Lambertian
                               light-mixture quirk makes most pixels of the bench frames NaN (C2 mid
                               rows, all of C4 at 1000 spp); with this flag the same launches carry
                               every sample's finite colour to a comparable output (and tier A's and
                               tier B's finite parts can be compared as distributions). */
#define RT_FLAG_SHARED_LIBM 8u /* tier A only, parity aid: sin, cos, log, atan, asin (and x ** 5) from the
                               portable include/rt_libm.h instead of the device's OCML, the functions the
                               oracle evaluates in the same mode. A column's tier-A stream is one serial
                               chain, so a last-bit difference between two libms that flips any later branch
                               changes the rest of the column; with one libm on both sides the streams are
                               compared bit for bit on every scene. */

typedef struct rt_render_params {
    int32_t width;
    int32_t height;
    int32_t spp;       /* numSamples */
    int32_t max_depth; /* maxDepth */
    int32_t rng_mode;  /* RT_RNG_EXACT | RT_RNG_PHILOX */
    uint32_t flags;
    uint64_t seed;       /* tier B Philox key */
    int32_t tile;        /* tile edge in pixels for sharding: a multiple of 8 in [8, 256] (0 = default 8) */
    int32_t shard_rank;  /* this shard (0-based) */
    int32_t shard_count; /* number of shards (GPUs); tiles are dealt round-robin */
    int32_t _pad;
} rt_render_params;

/* ------------------------------------------------------------------ version / errors */
int rt_abi_version(void);
const char* rt_last_error(void);

/* ------------------------------------------------------------------ RNG (src/Random.hs) */
/* randGen s = mkStdGen s  (src/Random.hs:20-21): writes (seed, gamma). */
void rt_rand_gen(int64_t s, uint64_t out_gen[2]);
/* randomDouble (src/Random.hs:23-25): one draw, advances gen in place. */
double rt_random_double(uint64_t gen[2]);

/* ------------------------------------------------------------------ scene construction */
/* A builder owns the RandGen threaded through scene construction (makeBVH / makePerlin
 * draw from it, src/Lib.hs:941-943, 424-439) and the growing record arrays. Object ids
 * returned by the constructors are node ids. */
typedef struct rt_builder rt_builder;

int rt_builder_create(const uint64_t gen[2], rt_builder** out);
void rt_builder_destroy(rt_builder* b);
/* Current generator state (the `g1` handed back by the Scenes.hs builders). */
void rt_builder_gen(const rt_builder* b, uint64_t out_gen[2]);

int rt_tex_constant(rt_builder* b, double r, double g, double bl);
int rt_tex_checker(rt_builder* b, int odd_tex, int even_tex);
int rt_tex_perlin(rt_builder* b, double scale); /* makePerlin: consumes 768 + 3*255 draws */
int rt_tex_image(rt_builder* b, const uint8_t* rgb, int width, int height); /* rgb NULL = Nothing */

int rt_mat_lambertian(rt_builder* b, int tex);
int rt_mat_metal(rt_builder* b, int tex, double fuzz);
int rt_mat_dielectric(rt_builder* b, double ref_idx);
int rt_mat_diffuse_light(rt_builder* b, int tex);
int rt_mat_isotropic(rt_builder* b, int tex);

int rt_obj_sphere(rt_builder* b, const double center[3], double radius, int mat);
int rt_obj_moving_sphere(rt_builder* b, const double c0[3], const double c1[3], double t0, double t1,
                         double radius, int mat);
/* plane: 0 = XYPlane, 1 = XZPlane, 2 = YZPlane (src/Lib.hs:649-660) */
int rt_obj_rect(rt_builder* b, int plane, double a0, double a1, double b0, double b1, double k, int mat);
int rt_obj_cuboid(rt_builder* b, const double pmin[3], const double pmax[3], int mat);
int rt_obj_translate(rt_builder* b, const double offset[3], int child);
int rt_obj_rotate(rt_builder* b, int axis, double angle_deg, int child);
int rt_obj_constant_medium(rt_builder* b, double density, int tex, int boundary);
int rt_obj_unhittable(rt_builder* b);
/* makeBVH mtime items (src/Lib.hs:941-961); has_time = 0 for Nothing. Consumes draws. */
int rt_obj_bvh(rt_builder* b, const int* items, int n_items, int has_time, double t0, double t1);

/* Seal the scene: world root, lights root (-1 = Unhittable), background. The descriptor
 * points into builder-owned memory and stays valid until the builder is destroyed. */
int rt_builder_finish(rt_builder* b, int world, int lights, const double background[3],
                      rt_scene_desc* out_desc);

/* Named scenes of src/Scenes.hs (ids below). `earth` = ImageTexture raster or NULL (Nothing).
 * The builder must be fresh; its generator is threaded as in the reference. */
enum rt_scene_id {
    RT_SCENE_CORNELL_BOX = 0,       /* makeCornellBoxScene        Scenes.hs:32-73   */
    RT_SCENE_CORNELL_SMOKE = 1,     /* makeCornellSmokeBoxScene   Scenes.hs:75-118  */
    RT_SCENE_SIMPLE_LIGHT = 2,      /* makeSimpleLightScene       Scenes.hs:133-155 */
    RT_SCENE_EARTH = 3,             /* makeEarthScene             Scenes.hs:167-179 */
    RT_SCENE_TWO_PERLIN_SPHERES = 4,/* makeTwoPerlinSpheresScene  Scenes.hs:194-211 */
    RT_SCENE_TWO_SPHERES = 5,       /* makeTwoSpheresScene        Scenes.hs:213-237 */
    RT_SCENE_RANDOM_BOOK_ONE = 6,   /* makeRandomSceneBookOne     Scenes.hs:253-317 */
    RT_SCENE_RANDOM = 7,            /* makeRandomScene            Scenes.hs:321-399 */
    RT_SCENE_NEXT_WEEK_FINAL = 8,   /* makeNextWeekFinalScene     Scenes.hs:414-466 */
    RT_SCENE_THREE_SPHERES = 9,     /* config 1: ground + s1..s3 of Scenes.hs:263-279, BVH (0,1) */
    RT_SCENE_STRESS_SPHERES = 10    /* config 5: `param` random spheres + ground, BVH (0,1) */
};
int rt_scene_named(rt_builder* b, int scene_id, double t0, double t1, const uint8_t* earth_rgb,
                   int earth_w, int earth_h, int64_t param, rt_scene_desc* out_desc);

/* newCamera lookfrom lookat vup vfov aspect aperture focusDist t0 t1 (src/Lib.hs:1269-1295). */
void rt_camera_new(const double lookfrom[3], const double lookat[3], const double vup[3], double vfov,
                   double aspect, double aperture, double focus_dist, double t0, double t1,
                   rt_camera* out);
enum rt_camera_id {
    RT_CAM_CORNELL = 0,      /* cornellCamera             Scenes.hs:120-131 */
    RT_CAM_TWO_SPHERES = 1,  /* twoSpheresSceneCamera     Scenes.hs:181-192 */
    RT_CAM_RANDOM_SCENE = 2, /* randomSceneCamera         Scenes.hs:239-250 */
    RT_CAM_NEXT_WEEK = 3     /* nextWeekFinalSceneCamera  Scenes.hs:401-412 */
};
int rt_camera_named(int cam_id, int width, int height, rt_camera* out);

/* P3 PPM text exactly as app/Main.hs:59-61 + printRow/showRow (src/Lib.hs:299-305).
 * Writes at most cap bytes; *out_len = bytes required. */
int rt_write_ppm(const uint8_t* rgb, int width, int height, char* buf, size_t cap, size_t* out_len);
/* Float dump of the per-pixel averages (rt_render's out_linear, H*W*3 doubles, top row first) as PFM:
 * "PF\n<W> <H>\n-1.0\n" + little-endian float32 RGB, bottom row first (the PFM order); f64 != 0
 * writes doubles under the header "PF64" instead (lossless). Same buffer protocol as rt_write_ppm. */
int rt_write_pfm(const double* linear, int width, int height, int f64, char* buf, size_t cap, size_t* out_len);

/* ------------------------------------------------------------------ device path */
typedef struct rt_ctx rt_ctx;

int rt_device_count(int* out);
/* Bind one HIP device (one process per GPU). */
int rt_create(int device, rt_ctx** out);
/*
 * One context over n_devices GPUs, driven from one host thread ("rt_create(num_gpus)":
 * the ctx owns the devices and an RCCL communicator over them). devices: n_devices distinct HIP device
 * ids, or NULL for 0..n_devices-1; at most RT_MAX_DEVICES. RCCL ranks follow the list order.
 *   rt_upload_scene[_ex]: validates and prepares the scene once, then copies it to every device.
 *   rt_render, tier B: the image's tiles are dealt round-robin over the devices (shard r = the r-th
 *     device, the rt_render_shard_async layout with shard_count = n_devices), each device renders its
 *     slab on its own stream, the slabs are gathered to the first device with RCCL (ncclGather over
 *     xGMI, grouped over the devices' communicators), which assembles the image and copies it to the
 *     host. The bytes equal a one-device rt_render of the same params (tier B is shard-invariant).
 *   rt_render, tier A: the reference's per-column streams are one serial chain per column, so tier A
 *     does not shard: it renders on the first device.
 * Every other call on a multi-device ctx (the *_async building blocks, debug entries, counting
 * renders) acts on its first device. This replaces the reference's only parallelism, the row sparks
 * of runRender (src/Lib.hs:1519-1520), as called from app/Main.hs:50-58.
 */
#define RT_MAX_DEVICES 16
int rt_create_multi(int n_devices, const int* devices, rt_ctx** out);
/* Devices of a ctx: *out_n = count; out_devices (may be NULL) receives up to `cap` device ids. */
int rt_ctx_devices(const rt_ctx* ctx, int* out_n, int* out_devices, int cap);
/* Timing of the last rt_render on a ctx (HIP events on each device's launch stream), ms:
 * kernel_ms[r] = device r's render launches (chunk batches included), gather_ms = from the first
 * device's render end to the end of the RCCL gather on its stream (includes waiting for the slowest
 * device), assemble_ms = the assemble kernel, frame_ms = first launch to assembled image (before the
 * device-to-host copy). n_devices = 1 and gather_ms = 0 on a one-device ctx. device_allocs = device
 * allocations (hipMalloc) the call made over all the ctx's devices: the ctx keeps its frame buffers (slabs,
 * gathered slabs, image, chunk sums) and grows them on demand, so a repeated frame of one size makes none. */
typedef struct rt_frame_timing {
    int32_t n_devices;
    int32_t device_allocs;
    double kernel_ms[RT_MAX_DEVICES];
    double gather_ms;
    double assemble_ms;
    double frame_ms;
} rt_frame_timing;
int rt_last_frame_timing(rt_ctx* ctx, rt_frame_timing* out);
void rt_destroy(rt_ctx* ctx);
/* Copy a scene to device memory (caller-owned desc; arrays are copied). Validates it.
 * Every medium occurrence of the world tree becomes its own keyed record (RT_RNG_PHILOX above), and by
 * default the world tree is re-bounded by a binned-SAH BVH over the same leaves, media and instance
 * frames included (the trees inside frames re-bounded in their own coordinates), for traversal (closest
 * hits are tree-independent except for exact ties, which are redone on the caller's tree; DESIGN.md
 * §3); the lights tree is always the caller's. */
int rt_upload_scene(rt_ctx* ctx, const rt_scene_desc* desc);
#define RT_UPLOAD_REFERENCE_BVH 1u /* traverse the caller's (makeBVH's) world tree as is */
int rt_upload_scene_ex(rt_ctx* ctx, const rt_scene_desc* desc, uint32_t flags);
/* The rebuild rt_upload_scene applies, on the host: the node array with the new world BVH
 * appended (out_nodes NULL: size query) and the new world root (== the old one if ineligible). */
int rt_rebuild_bvh(const rt_scene_desc* desc, rt_node* out_nodes, int capacity, int* out_n, int* out_root);
/* The 4-wide collapse the device walk uses (rt_wide.h records, 128 B each) of the binary tree at
 * `root` of a node array (e.g. rt_rebuild_bvh's output): out NULL = size query. out_stack_need
 * = the walk's stack bound (entries). RT_E_UNSUPPORTED when the root is not a BVH node. */
int rt_wide_bvh(const rt_node* nodes, int n_nodes, int root, void* out, int capacity, int* out_n,
                int* out_stack_need);
/* The 64-byte quantised form (rt_qnode, rt_wide.h) of n 4-wide records (rt_wide_bvh output) that the
 * kernels reading the tree from global memory walk: out holds n records. RT_E_UNSUPPORTED when a node's
 * boxes cannot be put on an fp32 grid (planes beyond fp32 range). */
int rt_quantize_wide(const void* wnodes, int n, void* out);
/* The host half of rt_upload_scene, with no device: validates `desc` exactly as the upload does
 * (same error codes and rt_last_error text; RT_UPLOAD_REFERENCE_BVH as for the upload) and describes
 * the device copy it would upload. Malformed descriptors can be checked on a machine without a GPU. */
typedef struct rt_scene_info {
    int32_t n_nodes;         /* device node records (the caller's + the rebuilt tree) */
    int32_t n_wide_nodes;    /* 4-wide nodes (the world's, or the mixed walk's subtrees'; 0 = none) */
    int32_t n_leaves;        /* their leaf-table records */
    int32_t world_root;      /* the walked world tree's root (the rebuilt one's when rebuilt) */
    int32_t stack_need;      /* stack entries of the binary / mixed walk */
    int32_t wide_stack_need; /* stack entries of the 4-wide walk */
    uint32_t features;       /* scene feature bits (F_* in ray-tracing_amd/csrc/rt_layout.h) */
    uint32_t variant;        /* the render-kernel variant chosen for them */
    int32_t rebuilt_bvh;     /* the world tree was rebuilt (SAH, or skeleton + re-bounded subtrees) */
    int32_t mixed_wide;      /* media / frame world with 4-wide trees under its skeleton */
    int32_t replace_ok;      /* frames nest <= 4 deep: the ray-replacement loop applies */
    int32_t ref_walk;        /* media or frames: walked in the reference's order */
} rt_scene_info;
int rt_prepare_scene(const rt_scene_desc* desc, uint32_t flags, rt_scene_info* out);
/* Stack entries the binary walk over the tree at `root` needs (the bound rt_upload_scene sizes
 * the LDS stacks with): left-first for the caller's nodes, either child first for rebuilt
 * (RT_BVH_ORDERED) nodes, one entry per open instance frame. */
int rt_tree_stack_need(const rt_node* nodes, int n_nodes, int root, int* out_need);

/*
 * Blocking full-image render (replaces runRender, src/Lib.hs:1491).
 *   col_gens     tier A: 2*width words (seed, gamma) per column, column 0 first
 *                (app/Main.hs:47-49); ignored in tier B.
 *   out_rgb8     H*W*3 bytes, top row first (pixelPositions, src/Lib.hs:1488-1489).
 *   out_linear   optional H*W*3 doubles: the per-pixel average before albedoToColor.
 *   out_col_gens optional (tier A): generators after the last row, 2*width words.
 * shard_rank/shard_count in params are ignored (whole image).
 */
int rt_render(rt_ctx* ctx, const rt_camera* cam, const rt_render_params* p, const uint64_t* col_gens,
              uint8_t* out_rgb8, double* out_linear, uint64_t* out_col_gens);

/*
 * Multi-GPU building blocks (tier B only). The image is cut into tile x tile squares,
 * numbered row-major from the top-left; shard r owns tiles r, r+N, r+2N, ... and writes
 * them into a "slab": tiles_per_shard * tile * tile pixels, tile-major. Every shard's slab
 * has the same size (padded), so slabs can be all-gathered as-is.
 */
int rt_shard_geometry(const rt_render_params* p, int64_t* tiles_total, int64_t* tiles_per_shard,
                      int64_t* slab_pixels);
/* Render this shard into device buffers on `stream` (hipStream_t, NULL = default).
 * d_slab_rgb8: slab_pixels*3 bytes; d_slab_linear: slab_pixels*3 doubles or NULL.
 * Asynchronous: stream-ordered, returns after the launches are queued. */
int rt_render_shard_async(rt_ctx* ctx, const rt_camera* cam, const rt_render_params* p,
                          uint8_t* d_slab_rgb8, double* d_slab_linear, void* stream);
/* Scatter shard_count gathered slabs (concatenated, rank-major) into a H*W*3 device image. */
int rt_assemble_async(rt_ctx* ctx, const rt_render_params* p, const uint8_t* d_slabs_rgb8,
                      uint8_t* d_image_rgb8, void* stream);
/* Same for the optional linear (double) slabs. */
int rt_assemble_linear_async(rt_ctx* ctx, const rt_render_params* p, const double* d_slabs_linear,
                             double* d_image_linear, void* stream);

/*
 * Counting build of the tier-B render (same output, slower): device-measured work for the
 * roofline. out_work[0..7] = {segments traced, BVH box tests, leaf primitive tests,
 * instance/medium tests, light-pdf evaluations, Philox blocks, samples, 4-wide node visits}
 * for this shard; out_work[8..10] = wave time (s_memtime ticks, summed over waves) spent acquiring work and
 * starting samples / traversing / shading; out_work[11..13] (ray-replacement loop only) = live-lane
 * slots of 4-wide node steps, of leaf steps and of outer iterations (lane utilisation = work / slots);
 * out_work[14] = leaf tests that found a hit, out_work[15] = walks redone for an exact tie (worlds
 * with media or frames: samples redone) (replacement loop).
 */
int rt_render_work(rt_ctx* ctx, const rt_camera* cam, const rt_render_params* p, uint64_t out_work[16]);

/* The same counting render, plus a profile of the binary / mixed walk's steps (replacement loop over
 * worlds with media or frames, and Cornell-like worlds): out_prof[m] = wave time (s_memtime ticks)
 * of the steps whose lanes were at the set m of node kinds, out_prof[32 + m] = their count; kinds:
 * 1 BVH box, 2 4-wide node, 4 leaf (primitive or chain), 8 ConstantMedium, 16 instance frame. */
int rt_render_step_profile(rt_ctx* ctx, const rt_camera* cam, const rt_render_params* p, uint64_t out_work[16],
                           uint64_t out_prof[64]);

/* Timing of the last render launch on this ctx (HIP events on the launch stream), ms. */
int rt_last_kernel_ms(rt_ctx* ctx, double* out_ms);

/* Which kernel the last tier-B render launch on this ctx ran (kernel selection is per scene and
 * frame: DESIGN.md §3): feature variant (rt_layout.h F_* bits; 32768: the instantiation an adaptive frame's
 * launches run, which tests the frame's skip mask), loop (0 one sample per lane walk,
 * 1 ray replacement over the binary tree, 2 over the 4-wide tree), LDS-staged scene or global
 * memory, leaf table in LDS, waves per SIMD the instantiation targets, grid and block size, dynamic
 * LDS bytes per workgroup, work-items and samples per work-item. */
typedef struct rt_launch_info {
    uint32_t variant;
    int32_t loop;
    int32_t lds_staged;
    int32_t leaf_lds;
    int32_t waves;
    int32_t grid;
    int32_t block;
    int32_t dyn_lds_bytes;
    int64_t work_items;
    int32_t chunk;
    int32_t wide_nodes;  /* 4-wide nodes the launched walk uses: the 4-wide world tree (loop 2), or the
                            mixed walk's trees over re-bounded subtrees (loop 1, media / frame worlds) */
    int32_t chunk_batches; /* launches the frame's chunks were split into (chunk sums bounded per launch) */
    int32_t _pad;
} rt_launch_info;
int rt_last_launch(rt_ctx* ctx, rt_launch_info* out);

/*
 * First-hit feature buffers: per-pixel albedo, normal, depth and coverage of the primary hit, the guide images
 * of a frame (NaN-free on every bench frame, converged at a handful of samples). Tier B only.
 *
 * Definition. For image pixel (px, row) (row 0 = top, as rt_render's outputs) and sample index s, the primary
 * ray is the one rt_render traces for that sample: stream key = seed, counter {pair, s, pid, 0} with
 * pid = row*W + px; draws 0 and 1 are ru, rv; u = (px + ru)/W, v = ((H-1-row) + rv)/H; getRay then makes its own
 * draws (disk rejection pairs, then the time). The closest hit is taken in [kEps, +inf) exactly as the render's
 * first segment takes it: the same tie rule, the same keyed ConstantMedium draw at the stream position reached
 * (RT_RNG_PHILOX above), and RT_FLAG_REFERENCE_CULL is honoured. The sample's feature vector is 8 doubles:
 *   albedo[3]  on a hit, textureValue of the hit material's texture at the hit's (u, v, p) for Lambertian, Metal,
 *              DiffuseLight (front or back face) and Isotropic, (1,1,1) for Dielectric; on a miss the background;
 *   normal[3]  the hit record's normal as faceNormal leaves it (a medium hit keeps the reference's fixed normal);
 *              0 on a miss;
 *   depth      t * sqrt(dot(d, d)), with the project's dot order (x*x + y*y + z*z) and no contraction; 0 on a miss;
 *   hits       1.0 or 0.0.
 * sums[pixel][k] is the left fold, in sample order, of the vectors of samples first_sample .. first_sample +
 * n_samples - 1, starting from 0, or from the caller's buffer when `accumulate` is set. A plain sample-order fold,
 * unlike the image's chunk order: a lane holds a pixel's eight sums in registers for all its samples (no chunk
 * sums), the result does not depend on how a caller splits the sample range, and a progressive caller can add
 * [k0, k1) onto what it has. Of rt_render_params the pass reads width, height, seed, rng_mode, flags
 * (RT_FLAG_REFERENCE_CULL) and the shard fields; spp, max_depth and the NaN flags are not read.
 *
 * rt_render_features        blocking; sums is host memory, [H][W][RT_FEATURE_DOUBLES], read first when accumulating.
 * rt_render_features_async  the same pass queued on `stream` into device memory in image order (on the ctx's device).
 * RT_E_INVALID, before any HIP call: a null argument, rng_mode != RT_RNG_PHILOX, RT_FLAG_SHARED_LIBM,
 * shard_count > 1 (shards are out of scope here: a feature pass covers the whole image), first_sample < 0,
 * n_samples < 1, first_sample + n_samples beyond INT32_MAX, a frame of 2^32 pixels or more. RT_E_STATE without a
 * scene. A multi-device ctx runs the pass on its first device. The launch is ordered after the ctx's previous
 * tier-B launch and before its next, whichever streams they use; a feature pass between two renders leaves the
 * renders' bytes unchanged.
 * rt_last_feature_launch    which kernel form the last feature pass ran: variant = the walk's feature bits, loop =
 *                           2 the 4-wide walk (spheres-only worlds with a 4-wide tree), 1 the mixed resumable walk
 *                           (every other world whose frames nest at most 4 deep), 0 the recursive walk; LDS staging,
 *                           waves, grid, block, dynamic LDS bytes; work_items = the frame's 8x8 pixel blocks (a wave
 *                           folds one block at a time, a lane one pixel); chunk = 0, chunk_batches = 1.
 * rt_features_resolve       host only, no device: from sums of n_samples >= 1 samples over `pixels` >= 1 pixels,
 *                           albedo and normal = sum / n (one IEEE division, as the image's average; the normal is
 *                           not renormalised), depth = depth sum / hits (+inf where hits is 0), coverage = hits / n,
 *                           and the albedo's bytes through scaleColor (NaN -> 0). Every output may be NULL (skipped).
 */
#define RT_FEATURE_DOUBLES 8
#define RT_FEAT_ALBEDO 0
#define RT_FEAT_NORMAL 3
#define RT_FEAT_DEPTH 6
#define RT_FEAT_HITS 7
int rt_render_features(rt_ctx* ctx, const rt_camera* cam, const rt_render_params* p, int first_sample, int n_samples,
                       int accumulate, double* sums);
int rt_render_features_async(rt_ctx* ctx, const rt_camera* cam, const rt_render_params* p, int first_sample,
                             int n_samples, int accumulate, double* d_sums, void* stream);
int rt_last_feature_launch(rt_ctx* ctx, rt_launch_info* out);
int rt_features_resolve(const double* sums, int64_t pixels, int n_samples, double* out_albedo, double* out_normal,
                        double* out_depth, double* out_coverage, uint8_t* out_albedo_rgb8);

/*
 * Specular-chain feature buffers: the same guides seen through glass and in mirrors. A first-hit pass gives a glass
 * ball the albedo (1,1,1) and a mirror its own texture, with the sphere's normal and depth: smooth guides over
 * everything seen in or through the ball. A chain pass follows the sample's path through specular scatters and takes
 * the features at the first vertex that is not followed, the albedo multiplied by the attenuations on the way and
 * the depth measured as path length. The chain is the exact prefix of the path rt_render traces for that sample.
 *
 * Definition. The sample's stream, UV pair and getRay are the first-hit pass's (above). Start with thr = (1,1,1),
 * len = 0.0, b = 0 and ray = the primary ray, then repeat:
 *   1. the closest hit of `ray` in [kEps, +inf) exactly as the render's segment takes it: the same tie rule, the
 *      same keyed ConstantMedium draw at the stream position reached, RT_FLAG_REFERENCE_CULL honoured;
 *   2. a miss: the vector is (thr * background, 0,0,0, 0, 0), one multiplication per channel (vmul); the sample ends;
 *   3. len = len + t * sqrt(dot(d, d)) of this segment (the project's dot order, no contraction);
 *   4. the hit's material is followed when b < max_bounces and it is a Dielectric with RT_CHAIN_DIELECTRIC set, or
 *      a Metal with RT_CHAIN_METAL set and fuzz <= max_fuzz;
 *   5. not followed: a = the first-hit rule's albedo of this hit (textureValue for Lambertian, Metal, DiffuseLight on
 *      either face and Isotropic, (1,1,1) for Dielectric); the vector is (thr * a, n, len, 1.0) with n this hit's
 *      normal as faceNormal leaves it; the sample ends;
 *   6. followed: the scattered ray is, bit for bit, the one the render's scatter makes for this hit at this stream
 *      position: the same draws in the same order (Dielectric one, Metal two even at fuzz 0) and the same
 *      operations (Metal: reflect(unit(d), n) + fuzz * v as written, at fuzz 0 too: the sign of a zero component can
 *      differ); thr = thr * attenuation, ray = scattered, ++b.
 * max_depth is not read. The sums are the first-hit pass's left fold in sample order over the same 8 doubles, so
 * rt_features_resolve, rt_denoise* and rt_frame_denoise take chain sums unchanged; resolved depth is the mean path
 * length to the terminal hit. With max_bounces = 0 or flags = 0 every value is the first-hit pass's bit for bit
 * (1.0 * x is x, and 0.0 + x is x for the positive x a depth is).
 *
 * rt_render_features_chain, rt_render_features_chain_async   rt_render_features[_async] with a chain: the same
 *     contract (ordering through the ctx's tier-B launches, no effect on the renders around it, the first device of
 *     a multi-device ctx), the same kernel forms, reported by rt_last_feature_launch in the same way. RT_E_INVALID,
 *     before any HIP call: everything rt_render_features rejects, a null chain, max_bounces outside 0..64, unknown
 *     flag bits, max_fuzz negative or not finite.
 * rt_last_feature_chain   the exact counts of the ctx's last chain pass. It waits for that pass first (an event of
 *     the ctx's own, recorded behind it: the caller's stream need not outlive the call that queued the pass), so
 *     after an async pass it blocks until the pass has run. RT_E_STATE if no chain pass was made.
 *     ended_cap / samples tells a caller whether max_bounces is large enough.
 */
#define RT_CHAIN_DIELECTRIC 1u
#define RT_CHAIN_METAL      2u
#define RT_CHAIN_MAX_BOUNCES 64
typedef struct rt_feature_chain {
    int32_t  max_bounces;  /* 0..64: specular scatters followed at most */
    uint32_t flags;        /* RT_CHAIN_*: which materials are followed */
    double   max_fuzz;     /* a Metal is followed when its fuzz <= max_fuzz (>= 0, finite) */
} rt_feature_chain;        /* 16 bytes */
typedef struct rt_feature_chain_stats {
    int64_t samples;        /* pixels * n_samples */
    int64_t ended_surface;  /* terminal hit on a material that is never followed under these flags */
    int64_t ended_miss;
    int64_t ended_cap;      /* terminal hit on a material that would have been followed at b < max_bounces */
    int64_t bounces;        /* specular scatters followed, summed over the samples */
} rt_feature_chain_stats;   /* 40 bytes */
int rt_render_features_chain(rt_ctx* ctx, const rt_camera* cam, const rt_render_params* p, const rt_feature_chain* chain,
                             int first_sample, int n_samples, int accumulate, double* sums);
int rt_render_features_chain_async(rt_ctx* ctx, const rt_camera* cam, const rt_render_params* p,
                                   const rt_feature_chain* chain, int first_sample, int n_samples, int accumulate,
                                   double* d_sums, void* stream);
int rt_last_feature_chain(rt_ctx* ctx, rt_feature_chain_stats* out);

/*
 * Material-ID coverage buffers: per pixel, which share of its samples saw which material (an anti-aliased ID matte
 * in the Cryptomatte style). Tier B only. Material ids only: rt_scene_desc's material indices. (Object ids would
 * need a primitive id in the hit record, which the render kernels do not carry.) Every output is an integer or
 * one IEEE division of two integers, so host and device agree bit for bit.
 *
 * Sample id. For pixel pid = row*W + px and sample s the ray, the stream and the closest hit are the first-hit
 * feature pass's (rt_render_features: the same UV pair, getRay, tie rule and keyed medium draw;
 * RT_FLAG_REFERENCE_CULL is honoured). With chain == NULL the sample's id is the hit's material index, or
 * RT_ID_MISS on a miss. With a chain, the chain is followed exactly as rt_render_features_chain defines it (steps
 * 1-6 above) and the id is the material of the vertex where it ends (step 5), or RT_ID_MISS when it ends in a miss
 * (step 2); max_bounces = 0 or flags = 0 give the chain == NULL records bit for bit. A ConstantMedium's id is its
 * phase material.
 *
 * Record and fold. One rt_id_record per pixel, image order. Samples first_sample .. first_sample + n_samples - 1
 * are folded in sample order from a zero record, or from the caller's record with `accumulate`. Per sample id x:
 * the first slot with count > 0 and id == x has its count incremented; if there is none, the first slot with
 * count == 0 takes id = x, count = 1; if there is none, `other` is incremented; `samples` is incremented always.
 * So slots appear in order of first appearance, the record is the whole state (folding [a,b) and then [b,c) with
 * `accumulate` gives the record of [a,c) byte for byte), and while other == 0 the slots are the exact histogram of
 * the pixel's ids. Saturation: a record whose `samples` is UINT32_MAX is full, and a sample folded into it leaves it
 * unchanged (a guard on the device and in rt_ids_fold_host alike; one call folds at most INT32_MAX samples, so it
 * can only be reached by accumulating).
 *
 * rt_render_ids        blocking, records in host memory (read first with `accumulate`).
 * rt_render_ids_async  the same pass queued on `stream` into device memory. Both follow the feature passes'
 *     contract: ordered through the ctx's tier-B launches, no effect on the renders around them, the first device
 *     of a multi-device ctx, the same kernel forms, reported by rt_last_feature_launch. RT_E_INVALID, before any
 *     HIP call: everything rt_render_features rejects (shard_count > 1 included) and, with a non-null chain, what
 *     rt_render_features_chain rejects of it. RT_E_STATE without a scene. With a non-null chain
 *     rt_last_feature_chain reports the pass's counts as for a chain feature pass (a pass without a chain leaves
 *     the last chain pass's counts in place).
 * rt_ids_fold_host     host only: folds ids[0..n) in order into *rec by the rule above (n >= 0).
 * rt_ids_resolve       host only: per pixel the seven slots sorted by count descending, then id ascending:
 *     out_rank_ids[7*i + k], out_rank_cov[7*i + k] = count / samples (one division); a free slot gives RT_ID_MISS
 *     and 0.0; out_other_cov[i] = other / samples. A record with samples == 0 gives 0.0 for every coverage (no
 *     division is made). Any output may be NULL.
 * rt_ids_matte_host, rt_ids_matte (blocking, host arrays through the device), rt_ids_matte_async (device arrays, on
 *     `stream`, ordered like a feature pass)   the matte of a set of ids: `ids` is a host array in every variant,
 *     strictly ascending, 1 <= n_ids <= RT_ID_MATTE_MAX (else RT_E_INVALID; RT_ID_MISS is a legal member: the sky
 *     matte). cov = (sum of the counts of the used slots whose id is in the list) / samples, the integer sum first,
 *     then one division (0.0 when samples == 0); out_cov[i] = cov, out_u8[i] = (uint8_t)(cov * 255.0 + 0.5). Either
 *     output may be NULL, not both. Host and device run one per-pixel text and give equal bytes.
 * rt_ids_preview_host, rt_ids_preview (blocking), rt_ids_preview_async   a false-colour image of the records, 3 bytes
 *     per pixel. The colour of an id x is, per channel c = 0,1,2, ((rt_ids_fmix32(x) >> 8*c) & 255) / 255.0, and
 *     black for RT_ID_MISS; rt_ids_fmix32 is MurmurHash3's 32-bit finaliser (public domain): h ^= h >> 16,
 *     h *= 0x85ebca6b, h ^= h >> 13, h *= 0xc2b2ae35, h ^= h >> 16. Channel value = the sum over the slots k in slot
 *     order of (count_k / samples) * colour_k(c), from 0.0, no contraction; the byte as in the matte.
 */
#define RT_ID_SLOTS 7
#define RT_ID_MISS 0xFFFFFFFFu
#define RT_ID_MATTE_MAX 1024
typedef struct rt_id_record {
    uint32_t id[RT_ID_SLOTS];     /* 0 in a free slot */
    uint32_t count[RT_ID_SLOTS];  /* 0 = free */
    uint32_t other;               /* samples whose id found no slot */
    uint32_t samples;             /* samples folded in all */
} rt_id_record;                   /* 64 bytes: a feature vector's size, one contiguous store per lane */
int rt_render_ids(rt_ctx* ctx, const rt_camera* cam, const rt_render_params* p, const rt_feature_chain* chain,
                  int first_sample, int n_samples, int accumulate, rt_id_record* records);
int rt_render_ids_async(rt_ctx* ctx, const rt_camera* cam, const rt_render_params* p, const rt_feature_chain* chain,
                        int first_sample, int n_samples, int accumulate, rt_id_record* d_records, void* stream);
int rt_ids_fold_host(rt_id_record* rec, const uint32_t* ids, int64_t n);
int rt_ids_resolve(const rt_id_record* recs, int64_t pixels, uint32_t* out_rank_ids, double* out_rank_cov,
                   double* out_other_cov);
int rt_ids_matte_host(const rt_id_record* recs, int64_t pixels, const uint32_t* ids, int n_ids, double* out_cov,
                      uint8_t* out_u8);
int rt_ids_matte(rt_ctx* ctx, const rt_id_record* recs, int64_t pixels, const uint32_t* ids, int n_ids,
                 double* out_cov, uint8_t* out_u8);
int rt_ids_matte_async(rt_ctx* ctx, const rt_id_record* d_recs, int64_t pixels, const uint32_t* ids, int n_ids,
                       double* d_out_cov, uint8_t* d_out_u8, void* stream);
int rt_ids_preview_host(const rt_id_record* recs, int64_t pixels, uint8_t* out_rgb8);
int rt_ids_preview(rt_ctx* ctx, const rt_id_record* recs, int64_t pixels, uint8_t* out_rgb8);
int rt_ids_preview_async(rt_ctx* ctx, const rt_id_record* d_recs, int64_t pixels, uint8_t* d_out_rgb8, void* stream);

/*
 * Sharded feature and ID passes: the three passes above over one shard's slab, and the merge of the shards' slabs.
 * The image-order entries above keep rejecting shard_count > 1; these are the per-device building blocks, as
 * rt_render_shard_async and rt_assemble_async are for the render. Tier B only.
 *
 * Geometry. The shard is (tile, shard_rank, shard_count) of `p`, with the geometry of rt_shard_geometry
 * (shard_count 0 means 1). The slab holds slab_pixels records of 64 bytes (RT_FEATURE_DOUBLES doubles, or one
 * rt_id_record) in slab order: tile-major over the shard's tiles r, r+N, r+2N, ...; inside a tile its 8x8 pixel
 * blocks row-major; inside a block (row & 7) * 8 + (px & 7). With lt the tile's index in the shard, bpr = tile / 8 and
 * (bx, by) the pixel's block inside the tile,
 *     slot = lt * tile * tile + (by * bpr + bx) * 64 + (row & 7) * 8 + (px & 7),
 * the slot rt_assemble_async reads. slot >> 6 numbers the slab's blocks: a wave folds one block and stores its 64
 * records as one contiguous 4 KB run.
 * Slot content. The slot of an image pixel holds, byte for byte, what the image-order pass (rt_render_features_async,
 * rt_render_features_chain_async, rt_render_ids_async) writes for that pixel with the same seed, flags, chain,
 * sample range and `accumulate`: a sample's stream is keyed by pid = row*W + px and the sample index, so which
 * shard folds a pixel does not show. Accumulating reads the slot first.
 * Padding. Slots of no image pixel (tile overhang, tiles past the image's last) are neither read nor written, with
 * `accumulate` too. A shard that owns no tile returns RT_OK and writes nothing. shard_count == 1 is legal: the
 * one-shard slab.
 *
 * rt_render_features_shard_async  a first-hit pass (chain NULL) or a specular-chain pass over the slab, queued on
 *                                 `stream` into device memory on the ctx's device.
 * rt_render_ids_shard_async       the material-ID pass over the slab (chain may be NULL).
 * Ordering is the feature passes': after the ctx's previous tier-B launch and before its next, whichever streams they
 * use; renders around a slab pass keep their bytes. The kernel forms are the ones the image-order pass of the same
 * world takes. rt_last_feature_launch reports the form, with work_items = the shard's tiles inside the image x
 * (tile/8)^2 (for one shard at tile 8, the image-order pass's count; 0 for a shard that owns no tile). After a chain or
 * ID-chain pass rt_last_feature_chain reports this shard's counts, samples = the shard's image pixels x n_samples;
 * added over the shards they are the image-order pass's counts.
 * RT_E_INVALID, before any HIP call: everything the image-order entry rejects other than shard_count > 1; what
 * rt_shard_geometry rejects of tile, shard_rank and shard_count; a slab of 2^32 slots or more; a null slab pointer.
 * RT_E_STATE without a scene. A multi-device ctx runs the pass on its first device.
 *
 * rt_assemble_records_async  d_slabs: shard_count slabs concatenated rank-major; d_image: [H][W] records on the ctx's
 *                            device. A pure byte move, for doubles and ID records alike, queued on `stream`; it reads no
 *                            padding slot. Needs no scene. Of `p` it reads width, height, tile and shard_count.
 * rt_assemble_records_host   the same on the host, no device.
 */
int rt_render_features_shard_async(rt_ctx* ctx, const rt_camera* cam, const rt_render_params* p,
                                   const rt_feature_chain* chain, int first_sample, int n_samples, int accumulate,
                                   double* d_slab_sums, void* stream);
int rt_render_ids_shard_async(rt_ctx* ctx, const rt_camera* cam, const rt_render_params* p,
                              const rt_feature_chain* chain, int first_sample, int n_samples, int accumulate,
                              rt_id_record* d_slab_records, void* stream);
int rt_assemble_records_async(rt_ctx* ctx, const rt_render_params* p, const void* d_slabs, void* d_image, void* stream);
int rt_assemble_records_host(const rt_render_params* p, const void* slabs, void* image);

/*
 * Feature-guided denoiser: an edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) with SVGF-style variance
 * guidance over a linear image, its per-pixel standard error (optional) and the feature sums of a feature pass
 * (above). Tier-independent; every array is in image order (row 0 = top). fp64 throughout, no contraction, only
 * + - * /, sqrt, fabs and comparisons, so that the host function and the device kernels give the same bits; the
 * falloffs are compact rationals (no exp). One per-pixel text serves both (ray-tracing_amd/csrc/rt_denoise.h).
 *
 * Inputs per pixel p of an H x W image: color[p][3] (rt_render's out_linear, rt_frame_resolve's or
 * rt_checkpoint_resolve's), se[p][3] (rt_frame_error's map; the pointer may be NULL) and feature_sums[p][8] of
 * n = feature_samples >= 1 samples, exactly as rt_render_features wrote them.
 *
 * Guides, computed once: N = normal sum / n (not renormalised); Z = depth sum / hits, or 0.0 where hits == 0
 * (not rt_features_resolve's +inf); A_c = albedo sum_c / n, and a_c = A_c clamped to [1e-3, 1]:
 * A_c > 1e-3 ? (A_c < 1.0 ? A_c : 1.0) : 1e-3 (a NaN albedo: 1e-3). The upper bound keeps emitters, whose first-hit
 * "albedo" is their radiance, and the pixels on their edges in their own units: divided by a radiance they would all
 * be 1 and take up their darker neighbours, which the multiplication at the end would then scale up.
 * Variance: V = ((0.2126 e_r)^2 + (0.7152 e_g)^2) + (0.0722 e_b)^2, each term (k * e) * (k * e), with e_c = se_c, or
 * under RT_DENOISE_DEMODULATE in a valid pixel e_c = se_c / a_c, the standard error of the channel the filter
 * sees; V = 0.0 when se is NULL, when one of the pixel's three se channels is not finite, or when that sum is not
 * finite. Luminance L(c) = (0.2126 r + 0.7152 g) + 0.0722 b. "Finite" is |x| <= DBL_MAX. A pixel is valid when its
 * three colour channels, as its buffer holds them at that moment, are finite.
 *
 * Demodulation (RT_DENOISE_DEMODULATE): before the first iteration a valid pixel's colour becomes color_c / a_c;
 * after the last, a pixel valid then becomes c_c * a_c. An invalid pixel's channels are never touched by either
 * step (they are copied, bit for bit).
 *
 * Iteration i = 0 .. iterations - 1 (1..8) has stride s = 2^i and maps one buffer of (colour, V) per pixel to the
 * next (two buffers, ping-pong). For centre p = (x, y), the 25 taps are q = (x + s dx, y + s dy), dy outer and dx
 * inner, both from -2 to 2: this is the order of every sum below. A tap outside the image or invalid is skipped.
 * Per centre, one division each: rz = 1 / (sigma_depth * Z_p + 1e-12), rc = 1 / (sigma_color * sqrt(V_p) +
 * color_floor); rn = 1 / (sigma_normal * sigma_normal) is computed once per call on the host. With
 * f(x) = x < 1.0 ? (1 - x) * (1 - x) : 0.0 (a NaN x gives 0) and k = {3/8, 1/4, 1/16}, a tap's weight is
 *     w = ((h * w_n) * w_z) * w_c,     h = k[|dx|] * k[|dy|],
 *     w_n = f((((N_p - N_q)_x^2 + (N_p - N_q)_y^2) + (N_p - N_q)_z^2) * rn),
 *     w_z = f(|Z_p - Z_q| * rz),       w_c = f(|L(c_p) - L(c_q)| * rc),
 * w_c = 1.0 under RT_DENOISE_GUIDES_ONLY. The sums start at 0: acc_c += w * c_q (multiply, then add),
 * wsum += w, vacc += (w * w) * V_q. If wsum > 0 the pixel becomes c' = acc / wsum, V' = vacc / (wsum * wsum); if
 * not (no tap has weight, or a NaN) the pixel's four values pass through unchanged.
 * An invalid centre passes through unchanged (a NaN frame's NaN pixels stay NaN, bit for bit, and change no
 * neighbour, being skipped as taps), unless RT_DENOISE_FILL is set: then it runs the same sums with w_c = 1.0, and
 * with wsum > 0 it takes c' and V' and is valid from the next iteration on.
 *
 * Outputs: out_color[p][3]; out_rgb8 (optional) = out_color through scaleColor, as rt_features_resolve's albedo
 * bytes (NaN -> 0). Stats: pixels = H*W; invalid_in = pixels of `color` with a channel that is not finite;
 * invalid_out = the same count over out_color; filled = pixels invalid in `color` and valid in out_color; all
 * exact. kernel_ms = HIP-event time of the call's kernels (0 from the host function).
 *
 * rt_denoise_host   host only, no device: the definition, and the offline half of a checkpoint workflow
 *                   (rt_checkpoint_resolve's linear image, rt_checkpoint_error's map). se, out_rgb8 and stats may be
 *                   NULL. out_color must not overlap an input.
 * rt_denoise        the same on the ctx's device (a multi-device ctx: its first), host pointers, blocking; bit for
 *                   bit rt_denoise_host's outputs and counts. Needs a ctx but no scene.
 * rt_denoise_async  the kernels queued on `stream` over device pointers in image order (d_se and d_out_rgb8 may be
 *                   NULL); composes with rt_render_features_async. The inputs are read until the last kernel ends.
 * rt_frame_denoise  an unsharded frame's current preview (rt_frame_resolve's S / N_p), with its rt_frame_error map
 *                   when the frame tracks moments and chunks_done >= 2 (else no se), denoised on the device against
 *                   d_feature_sums (device memory, [H][W][8], e.g. rt_render_features_async's); only the result is
 *                   copied back (out_rgb8, out_linear, stats: each may be NULL). params->width and height must be
 *                   the frame's. The frame's sums, its stored preview and its bytes_changed accounting are left
 *                   alone. RT_E_STATE: no scene, no chunk rendered, or a shard frame (a sharded denoise needs a halo
 *                   exchange between the shards, which is not covered).
 * rt_last_denoise   of the ctx's last denoise call: device_allocs = device allocations it made (the ctx keeps the
 *                   guide records, the two (colour, V) buffers and its staging buffers and grows them on demand, so
 *                   a repeat of one image size makes none); launches = kernels queued (iterations + 2); lds_bytes =
 *                   the iteration kernel's LDS per workgroup.
 * RT_E_INVALID, before any HIP call: a null required pointer; width or height < 1; iterations outside 1..8;
 * feature_samples < 1; unknown flag bits; sigma_color, sigma_normal, sigma_depth or color_floor not > 0 or not
 * finite; an image of 2^31 pixels or more. The kernels are ordered after the ctx's previous tier-B launch and
 * before its next, whichever streams they use; a denoise between two renders leaves the renders' bytes unchanged.
 */
#define RT_DENOISE_DEMODULATE 1u  /* filter colour / albedo, multiply the albedo back at the end */
#define RT_DENOISE_GUIDES_ONLY 2u /* w_c = 1: normal and depth weights only */
#define RT_DENOISE_FILL 4u        /* replace invalid (NaN, infinite) pixels by their valid neighbourhood */
#define RT_DENOISE_MAX_ITERATIONS 8
typedef struct rt_denoise_params {
    int32_t width;
    int32_t height;
    int32_t iterations;      /* 1..8; iteration i has stride 2^i */
    int32_t feature_samples; /* n of feature_sums */
    uint32_t flags;          /* RT_DENOISE_* */
    int32_t _pad;
    double sigma_color;  /* in standard errors of the centre's luminance */
    double color_floor;  /* added to sigma_color * sqrt(V_p): the luminance scale where V is 0 */
    double sigma_normal; /* |N_p - N_q| at which w_n reaches 0 */
    double sigma_depth;  /* |Z_p - Z_q| / Z_p at which w_z reaches 0 */
} rt_denoise_params; /* 56 bytes */
typedef struct rt_denoise_stats {
    int64_t pixels;
    int64_t invalid_in;
    int64_t invalid_out;
    int64_t filled;
    double kernel_ms;
} rt_denoise_stats; /* 40 bytes */
typedef struct rt_denoise_info {
    int32_t device_allocs;
    int32_t launches;
    int32_t lds_bytes;
    int32_t _pad;
} rt_denoise_info; /* 16 bytes */
int rt_denoise_host(const rt_denoise_params* params, const double* color, const double* se,
                    const double* feature_sums, double* out_color, uint8_t* out_rgb8, rt_denoise_stats* stats);
int rt_denoise(rt_ctx* ctx, const rt_denoise_params* params, const double* color, const double* se,
               const double* feature_sums, double* out_color, uint8_t* out_rgb8, rt_denoise_stats* stats);
int rt_denoise_async(rt_ctx* ctx, const rt_denoise_params* params, const double* d_color, const double* d_se,
                     const double* d_feature_sums, double* d_out_color, uint8_t* d_out_rgb8, void* stream);
int rt_last_denoise(rt_ctx* ctx, rt_denoise_info* out);

/*
 * Progressive tier-B frames: the image of rt_render, rendered a few sample chunks at a time.
 * A frame holds the running per-pixel sums of the chunks rendered so far (RT_RNG_PHILOX above: chunk
 * sums added in chunk order from 0), so that a caller can look at the image while it converges, stop
 * when it is good enough, or save the sums and finish the frame later. A frame advanced to its end in
 * any step pattern resolves to the bytes and the linear image of rt_render with the same params.
 *
 * open     Tier B only (RT_RNG_EXACT: RT_E_UNSUPPORTED, a column's stream is one serial chain). The
 *          frame is the whole image (shard_rank / shard_count are ignored, as in rt_render); on a
 *          multi-device ctx it acts on the first device. The chunk size is fixed here:
 *          CH = rt_sample_chunk(width*height, spp), chunks_total = ceil(spp / CH). The frame owns its
 *          running sums (device memory, 24 bytes per pixel of the tile-padded image); the chunk sums
 *          of a launch, the tail buffer and the work counter stay the ctx's. rt_render,
 *          rt_render_shard_async and the debug entries may be called on the ctx between two advances:
 *          they neither disturb the frame nor change their own results. Several frames may be open.
 * advance  Renders the next min(max_chunks, remaining) chunks in chunk order and adds their sums to the
 *          running sums, the same additions in the same order as rt_render makes. *out_chunks_done_now
 *          (may be NULL) = chunks rendered by this call; 0 on a complete frame is not an error. A step
 *          whose chunk sums exceed the per-launch bound is split into launches as a whole frame is.
 *          Asynchronous: returns once the launches are queued; resolve and save drain them.
 * resolve  The image over the samples rendered so far: per pixel sum / samples_done, then
 *          albedoToColor; on a complete frame, rt_render's output bit for bit. out_rgb8 (H*W*3 bytes),
 *          out_linear (H*W*3 doubles) and out may each be NULL: a null image pointer skips that copy,
 *          so stats alone are a cheap poll. RT_E_STATE before the first chunk is rendered.
 * stats    chunk = CH; chunks_total; chunks_done; samples_done = min(spp, chunks_done * CH);
 *          kernel_ms = HIP-event time of the render launches queued since the last resolve;
 *          nan_pixels = image pixels whose running sum has a NaN channel (permanent: the reference's
 *          Lambertian-mixture quirk; their bytes stay 0); bytes_changed = 8-bit channels that differ
 *          from the previous resolve of this frame (the first resolve of an opened or restored frame
 *          compares with an all-zero image): the stopping rule of an 8-bit output is "the bytes
 *          stopped moving". Both counts are exact.
 * lifetime rt_upload_scene[_ex] on the ctx invalidates its open frames: their advance, resolve and
 *          save return RT_E_STATE, close still works. rt_destroy closes the frames still open (their
 *          handles are dead afterwards).
 * save     The frame as a blob (below), with rt_write_ppm's buffer protocol: *out_len = bytes
 *          required; the blob is written when cap >= *out_len (buf NULL or a short cap: size query).
 * restore  A new frame from a blob, continuing exactly where the saved one stopped. RT_E_INVALID for
 *          a malformed blob (rt_frame_blob_info's checks), RT_E_STATE when the ctx has no scene or
 *          its scene's fingerprint or upload flags differ from the blob's.
 *
 * Blob layout, little-endian, RT_FRAME_BLOB_HEADER = 288 bytes of header, then the payload:
 *     0  8 bytes  magic "RTFRAME\0"
 *     8  u32      blob version (RT_FRAME_BLOB_VERSION = 1)
 *    12  u32      upload flags of the scene (rt_upload_scene_ex)
 *    16  48 bytes rt_render_params: i32 width, height, spp, max_depth, rng_mode; u32 flags; u64 seed;
 *                 i32 tile, shard_rank, shard_count, _pad
 *    64 192 bytes rt_camera: 24 f64 in declaration order
 *   256  i32      CH
 *   260  i32      chunks_done
 *   264  i64      pixel count (width * height)
 *   272  u64      scene fingerprint: 64-bit FNV-1a over the bytes of the caller's node, material,
 *                 texture, perlin, image and image-pool arrays, then world_root, lights_root (i32)
 *                 and background (3 f64) of the rt_scene_desc uploaded
 *   280  u64      payload bytes = pixel count * 24
 *   288  payload  the running sums, 3 f64 per pixel, image order (top row first)
 * rt_frame_blob_info checks, on the host alone: the length covers the header; magic; version; width,
 * height, spp positive (spp at most 2^31 - 1 - RT_CHUNK_MAX), max_depth >= 0, rng_mode
 * RT_RNG_PHILOX, tile 0 or a multiple of 8 in [8, 256]; pixel count = width * height < 2^32;
 * CH = rt_sample_chunk(pixels, spp); 0 <= chunks_done <= chunks_total; payload bytes = pixels * 24;
 * length = 288 + payload bytes. Else RT_E_INVALID.
 *
 * Per-pixel error estimates (frames opened with RT_FRAME_MOMENTS). A pixel's samples are independent
 * Philox streams, so the spread of its chunk sums estimates its variance (batch means). Besides the
 * running sum S = sum_k S_k, a tracked frame keeps per pixel and channel
 *     Q = sum_k (S_k * S_k) / (double)n_k,   added in chunk order from 0,
 * S_k chunk k's sum and n_k its sample count (CH, or fewer for the short last chunk; k is the frame's
 * chunk index). Each term is computed as written in IEEE fp64: multiply, divide, then add (no
 * contraction). Like the sums, Q is a fixed function of (scene, camera, params), independent of step
 * pattern and chunk batching, and tracking changes no sum: a tracked frame's image and blob are the
 * untracked frame's bit for bit. After K >= 2 chunks and N samples, per channel, in this order:
 *     t = (S * S) / N;   d = Q - t, set to 0 when d < 0 (rounding only);   se = sqrt((d / (K - 1)) / N)
 * se is the standard error of the pixel's mean S / N; the estimate of the variance under it is unbiased,
 * E[sum_k S_k^2 / n_k - S^2 / N] = (K - 1) sigma^2. A pixel is non-finite when any se channel is not
 * finite (NaN sums of the Lambertian-mixture quirk, infinite sums). A finite pixel is converged under
 * (abs_tol, rel_tol) when se_c <= abs_tol + rel_tol * |S_c / N| holds for all three channels.
 *
 * open_ex     rt_frame_open with frame flags (rt_frame_open = flags 0; unknown bits: RT_E_INVALID). With
 *             RT_FRAME_MOMENTS the frame also owns Q (device memory, slab order, zeroed, 24 bytes per
 *             pixel of the tile-padded image) and advance folds the Q terms with the sums.
 * moments     Q in image order, H*W*3 doubles (drains the frame's queued work). RT_E_STATE when the frame
 *             does not track moments or no chunk has been rendered.
 * restore_ex  rt_frame_restore plus the moments saved with the blob (H*W*3 doubles, image order, as
 *             rt_frame_moments wrote them when the blob was saved): a tracked frame that continues exactly
 *             where the saved one stopped. moments == NULL: rt_frame_restore (an untracked frame). The
 *             version-1 blob has no room for Q and is unchanged; keeping a blob and its moments together
 *             is the caller's responsibility (moments of another save give a frame whose Q is not rt.h's);
 *             a checkpoint (below) holds both.
 * error       The error map and its summary at any point of a tracked frame with chunks_done >= 2, at a
 *             tolerance (NULL: {0, 0}; a negative or NaN value: RT_E_INVALID). out_se (H*W*3 doubles, image
 *             order) and out may each be NULL. RT_E_STATE for an untracked frame, a frame whose ctx's
 *             scene was replaced, or chunks_done < 2. Independent of rt_frame_resolve: it leaves
 *             bytes_changed and the stored preview alone.
 * error stats pixels = H*W; nonfinite_pixels; unconverged_pixels counts finite pixels only; max_se and
 *             mean_se run over the channels of finite pixels (0 when there are none). The counts and
 *             max_se are exact. mean_se is added in a fixed order without floating-point atomics, so
 *             every call returns the same value; it agrees with the sequential fp64 sum to 1e-12 relative.
 * rt_error_estimate  The same per-pixel function on the host alone (no device), over image-order arrays:
 *             an error map offline from a blob's payload and the saved moments. mean_se is the
 *             sequential sum in pixel and channel order. chunks_done < 2, pixels <= 0, samples_done <
 *             chunks_done, a null array or a bad tolerance: RT_E_INVALID.
 *
 *
 * Adaptive frames: stopping pixels. A frame becomes adaptive through calls (rt_frame_adapt, rt_frame_stop),
 * not through an open flag; a frame on which neither is made renders exactly as above.
 *   - Each pixel of a frame is active or stopped. Stopping is permanent.
 *   - A pixel stopped when the frame had K_p chunks done keeps its S and Q from that moment: the sums of
 *     chunks 0..K_p-1 of the tier-B definition, bit for bit the values an unadapted frame of the same
 *     (scene, camera, params) holds after K_p chunks. For an active pixel K_p = chunks_done.
 *   - N_p = min(spp, K_p * CH). Resolve gives S_p / N_p. rt_frame_error uses (K_p, N_p) per pixel; a pixel
 *     with K_p < 2 is non-finite (its se channels are NaN).
 *   - rt_frame_advance renders the next chunks for active pixels only. With no active pixel it renders
 *     nothing and reports 0 chunks, as on a complete frame (chunks_done stays).
 *   - The image is a fixed function of (scene, camera, params, and the sequence of stop calls, each with the
 *     chunks_done it was made at). It does not depend on the step pattern between stop calls, on chunk
 *     batching, or on other calls interleaved on the ctx.
 * adapt       Applies a rule on the device to the active pixels at the frame's current (K, N) = (chunks_done,
 *             samples_done). With RT_ADAPT_NAN a pixel whose S has a NaN channel stops (resolve's nan_pixels:
 *             such a sum never recovers, its bytes are 0 and its linear value NaN whatever is added, so with
 *             RT_ADAPT_NAN alone the finished image is rt_render's bit for bit). Otherwise, with
 *             RT_ADAPT_CONVERGED, a pixel stops when K >= max(2, min_chunks) and it is converged under
 *             (abs_tol, rel_tol) by rt_frame_error's rule. Pixels with infinite sums never stop. RT_E_INVALID:
 *             flags 0 or unknown bits, a negative or NaN tolerance, min_chunks < 2 with RT_ADAPT_CONVERGED.
 *             RT_E_STATE: no chunk rendered yet, a frame whose ctx's scene was replaced, RT_ADAPT_CONVERGED on
 *             a frame without moments. RT_ADAPT_NAN alone needs only S and works on untracked frames.
 *             Stopping on an estimated error biases the stopped pixels: the chunks that looked quiet are the
 *             ones kept (a pixel whose first chunks happen to agree stops on too small an estimate).
 *             min_chunks is the guard.
 * stop        The caller's own rule: mask holds H*W bytes in image order, nonzero = stop that pixel now (a
 *             pixel already stopped stays as it is). Works on untracked frames. RT_E_STATE as for adapt.
 * adapt stats pixels = H*W; active_pixels; stopped_nan = stopped pixels whose S has a NaN channel;
 *             stopped_converged_or_masked = the other stopped pixels; stopped_now = this call's. All exact.
 *             `out` may be NULL.
 * chunk_counts K_p per pixel, H*W int32 in image order (an active pixel: chunks_done).
 * save        rt_frame_save on a frame with any stopped pixel returns RT_E_STATE: the version-1 blob has no
 *             room for K_p and stays as it is (rt_frame_checkpoint, below, saves such a frame).
 *             rt_frame_moments still works on an adapted frame.
 * rt_adapt_decide  The same per-pixel rule on the host alone (no device), over image-order arrays (a blob's
 *             payload and the saved moments at `chunks_done` chunks of a frame of chunk size `chunk`):
 *             chunks_out[i] = chunks_in[i] where that is nonzero (already stopped), chunks_done where the
 *             rule stops pixel i now, else 0 (active). moments may be NULL for a rule without
 *             RT_ADAPT_CONVERGED; chunks_in may be NULL (no pixel stopped yet); chunks_out may be chunks_in;
 *             one of chunks_out and out may be NULL. The stats classify stopped pixels by the sums passed.
 *             RT_E_INVALID: a null sums or rule, a bad rule, pixels < 1, chunks_done outside
 *             [1, ceil(spp / chunk)], a chunks_in value outside [0, chunks_done].
 *
 * Shard frames: a progressive frame over the slab of (tile, shard_rank, shard_count), the tile shard of
 * rt_render_shard_async. Its sums, moments, K_p, previews and error map are per slab pixel, and its outputs
 * are slabs left in device memory, so the gather of the caller's choice and rt_assemble[_linear]_async merge
 * N shard frames into exactly what an unsharded frame of the same (scene, camera, params, stop calls) gives,
 * bit for bit (tier B is shard-invariant). The frames of one image may live on different ctxs, devices or
 * processes; each is advanced, adapted and stopped on its own, and they agree as long as the callers make the
 * same stop calls at the same chunks_done. Slots of a slab outside the image (tile padding, and the tiles past
 * the last one when shard_count does not divide the tile count) are never read by assemble: their content
 * in every output below is unspecified.
 * open_shard     rt_frame_open_ex that honours p->tile, p->shard_rank and p->shard_count (checked as
 *                rt_shard_geometry checks them; RT_E_INVALID). CH and chunks_total are the whole image's
 *                (rt_sample_chunk(width*height, spp)). The frame owns slab_pixels of sums, and of Q with
 *                RT_FRAME_MOMENTS. Tier A: RT_E_UNSUPPORTED. A frame opened this way is a shard frame even at
 *                shard_count 1. On a multi-device ctx it acts on the first device.
 * advance        As above, over the shard's tiles. A shard that owns no image pixel (more shards than tiles)
 *                launches nothing and still counts the chunks.
 * resolve_shard  The preview over the samples so far into caller device buffers: d_slab_rgb8 slab_pixels*3
 *                bytes, d_slab_linear slab_pixels*3 doubles; either may be NULL, both NULL is a stats poll.
 *                Blocking. nan_pixels and bytes_changed count the shard's own image pixels (the frame keeps its
 *                previous preview in slab order); summed over the shards they are the unsharded frame's counts.
 * error_shard    rt_frame_error's map (d_slab_se: slab_pixels*3 doubles of device memory, may be NULL) and
 *                summary over the shard's pixels, per pixel at (K_p, N_p). pixels = the image pixels the shard
 *                owns. Counts and max_se are exact; mean_se is added in a fixed order with no floating-point
 *                atomics, so every call returns the same value.
 * merging stats  rt_error_stats_merge (host only): counts are added, max_se is the maximum, mean_se is the mean
 *                weighted by finite pixels, sum_r mean_r * (pixels_r - nonfinite_r) / sum_r (pixels_r -
 *                nonfinite_r), or 0 when there are none; it agrees with rt_error_estimate over the whole image
 *                to 1e-12 relative. RT_E_INVALID when the parts disagree in chunks_done or samples_done.
 *                rt_frame_stats and rt_adapt_stats of the shards merge by plain addition of their counts
 *                (nan_pixels, bytes_changed; pixels, active_pixels, stopped_nan, stopped_converged_or_masked,
 *                stopped_now); kernel_ms is per shard.
 * adapt, stop    Work on shard frames as above: stop takes the same image-order H*W mask and reads only the
 *                shard's own pixels; the stats are over the shard's pixels (pixels = owned image pixels).
 * shard_state    Device copies of S and Q (3 doubles per slab pixel) and K_p (int32 per slab pixel; an active
 *                pixel: chunks_done) in slab order; each pointer may be NULL. d_slab_moments on an untracked
 *                frame: RT_E_STATE. Blocking.
 * save_header    The 288-byte header of the frame's whole-image version-1 blob (cap >= RT_FRAME_BLOB_HEADER, else
 *                RT_E_INVALID): the shard fields are written as 0 / 1, every other field as rt_frame_save writes
 *                it, so the header is the same on every shard. The caller appends the assembled image-order
 *                sums (shard_state's S through rt_assemble_linear_async): header + sums is the unsharded frame's
 *                blob byte for byte. RT_E_STATE on a frame with stopped pixels, as save. Works on unsharded
 *                frames too.
 * restore_shard  A shard frame (shard_rank of shard_count) from a whole-image version-1 blob, the tile being the
 *                blob's; `moments` (optional) is image order, H*W*3 doubles, as for restore_ex. Only the owned
 *                pixels are taken. The payload is tile-independent, so a checkpoint of N shards resumes on M.
 *                Fingerprint and upload-flag checks as rt_frame_restore.
 * kinds          rt_frame_resolve, rt_frame_save, rt_frame_moments, rt_frame_chunk_counts and rt_frame_error
 *                return RT_E_STATE on a shard frame (the message names the call to use); resolve_shard,
 *                error_shard and shard_state return RT_E_STATE on an unsharded frame.
 *
 * Checkpoints: the version-2 blob, which carries a tracked frame's Q and an adapted frame's K_p with the sums,
 * so that any frame can be interrupted and continued. The version-1 calls above are unchanged: rt_frame_save
 * writes and rt_frame_restore* and rt_frame_blob_info take version 1 only. Layout, little-endian,
 * RT_FRAME_CKPT_HEADER = 320 bytes of header, then the payload:
 *     0..287   the version-1 header, field for field, with version = 2 (RT_FRAME_CKPT_VERSION); the u64 at 280 =
 *              the bytes that follow offset 320
 *   288  u32   sections: RT_CKPT_MOMENTS (1) | RT_CKPT_STOPS (2); any other bit is invalid
 *   292  28 bytes reserved, all zero (a nonzero byte is invalid)
 *   320        S  pixels * 3 f64, image order (as version 1)
 *              Q  pixels * 3 f64, image order, only with RT_CKPT_MOMENTS
 *              K  pixels * i32, image order, only with RT_CKPT_STOPS: 0 = an active pixel, else K_p in
 *                 [1, chunks_done]
 * K stores 0 for an active pixel, unlike rt_frame_chunk_counts, whose chunks_done for an active pixel cannot be
 * told from a pixel stopped at the current chunks_done. The header holds no counts: every shard of an image
 * writes the same bytes.
 * checkpoint_info  (host only) Parses and validates a version-1 or version-2 blob. desc.blob is
 *             rt_frame_blob_info's descriptor (payload_bytes = the bytes after the blob's own header); a
 *             version-1 blob has sections 0. sums_offset, moments_offset and stops_offset are byte offsets
 *             from the start of the blob (0: the section is absent). stopped_pixels (K != 0), stopped_nan
 *             (those whose S has a NaN channel) and active_pixels are counted by scanning the payload. Checks:
 *             every version-1 rule, the section bits, the reserved bytes, payload bytes = pixels *
 *             (24 + 24 [Q] + 4 [K]), length = 320 + payload bytes, every K in [0, chunks_done]. Else RT_E_INVALID.
 * checkpoint_resolve  (host only) The preview rt_frame_resolve gives of that state, by the device's arithmetic:
 *             per pixel S / N_p, N_p = min(spp, K_p * CH) for a stopped pixel, else the frame's samples_done,
 *             then albedoToColor. out_rgb8 (H*W*3 bytes), out_linear (H*W*3 doubles) and out may each be NULL.
 *             nan_pixels is exact, bytes_changed is taken against an all-zero image, kernel_ms is 0.
 *             RT_E_INVALID for a malformed blob or chunks_done = 0.
 * checkpoint_error  (host only) rt_frame_error's map and summary of that state, per pixel at (K_p, N_p) by
 *             rt_error.h's function; mean_se is the sequential sum in pixel and channel order. RT_E_INVALID for a
 *             malformed blob, one without RT_CKPT_MOMENTS, chunks_done < 2 or a bad tolerance.
 * checkpoint  rt_frame_save's buffer protocol on an unsharded frame; always version 2. RT_CKPT_MOMENTS is set if
 *             and only if the frame tracks moments, RT_CKPT_STOPS if and only if at least one pixel is stopped
 *             (when rt_frame_save refuses). With sections 0 the blob is rt_frame_save's apart from the version
 *             word and the 32 further header bytes. RT_E_STATE on a shard frame.
 * resume      A new frame from a version-1 or version-2 blob: the saved frame. It tracks moments if and only if
 *             the blob has Q, and has stopped pixels if and only if the blob has K with a nonzero entry. Any
 *             further sequence of advance, adapt, stop, resolve, error, moments, chunk_counts and checkpoint calls
 *             gives, bit for bit and count for count, what the uninterrupted frame gives (but the first resolve's
 *             bytes_changed is taken against zero, as for every restored frame). Errors as rt_frame_restore.
 * resume_shard  The same as a shard frame (shard_rank of shard_count, the tile being the blob's): only the owned
 *             pixels are taken, so a checkpoint of N shards resumes on M, or unsharded.
 * shard_stops The raw K_p of a shard frame (0 = active) in slab order into device memory, slab_pixels int32: all
 *             zeros before any stop call; padding slots unspecified. RT_E_STATE on an unsharded frame.
 * checkpoint_header  The 320 header bytes of the whole image's checkpoint (cap >= RT_FRAME_CKPT_HEADER, else
 *             RT_E_INVALID), the shard fields written as 0 / 1. `sections` is the caller's, the OR over the
 *             image's shards (unknown bits: RT_E_INVALID; RT_CKPT_MOMENTS on an untracked frame: RT_E_STATE).
 *             `chunks_done` is the image's (-1: the frame's own): a shard whose pixels are all stopped may lag
 *             behind the others, so a value above the frame's own is accepted when the frame has no active
 *             pixel (else RT_E_STATE); a value below the frame's own or above chunks_total is RT_E_INVALID.
 *             Header + assembled S + assembled Q + merged K is the unsharded frame's checkpoint byte for byte.
 *
 * Not covered: frames spanning the devices of an rt_create_multi ctx (a shard frame acts on one device; the
 * caller gathers), reactivating a stopped pixel, adaptive one-shot rt_render, compacting a mostly stopped
 * frame's work-items, error estimates and adaptive sampling for tier A, a checksum over a blob's payload, and
 * extending a frame past its spp (CH depends on spp). RT_FLAG_NAN_CULL keeps its per-chunk meaning.
 */
#define RT_FRAME_BLOB_VERSION 1u
#define RT_FRAME_BLOB_HEADER 288
#define RT_FRAME_CKPT_VERSION 2u
#define RT_FRAME_CKPT_HEADER 320
#define RT_CKPT_MOMENTS 1u /* the checkpoint has Q */
#define RT_CKPT_STOPS 2u   /* the checkpoint has K */
typedef struct rt_frame rt_frame;
typedef struct rt_frame_stats {
    int32_t chunk;
    int32_t chunks_total;
    int32_t chunks_done;
    int32_t samples_done;
    double kernel_ms;
    int64_t nan_pixels;
    int64_t bytes_changed;
} rt_frame_stats; /* 40 bytes */
typedef struct rt_frame_blob_desc {
    uint32_t version;
    uint32_t upload_flags;
    rt_render_params params;
    rt_camera camera;
    int32_t chunk;
    int32_t chunks_total;
    int32_t chunks_done;
    int32_t samples_done;
    int64_t pixels;
    uint64_t scene_fingerprint;
    uint64_t payload_bytes;
} rt_frame_blob_desc; /* 288 bytes */
int rt_frame_open(rt_ctx* ctx, const rt_camera* cam, const rt_render_params* p, rt_frame** out);
int rt_frame_advance(rt_frame* f, int max_chunks, int* out_chunks_done_now);
int rt_frame_resolve(rt_frame* f, uint8_t* out_rgb8, double* out_linear, rt_frame_stats* out);
int rt_frame_save(rt_frame* f, void* buf, size_t cap, size_t* out_len);
int rt_frame_restore(rt_ctx* ctx, const void* buf, size_t len, rt_frame** out);
int rt_frame_blob_info(const void* buf, size_t len, rt_frame_blob_desc* out);
void rt_frame_close(rt_frame* f);
#define RT_FRAME_MOMENTS 1u /* frame flag: keep Q, the per-pixel second moment of the chunk sums (above) */
typedef struct rt_error_tol {
    double abs_tol;
    double rel_tol;
} rt_error_tol; /* 16 bytes */
typedef struct rt_error_stats {
    int32_t chunks_done;
    int32_t samples_done;
    int64_t pixels;
    int64_t nonfinite_pixels;
    int64_t unconverged_pixels;
    double max_se;
    double mean_se;
} rt_error_stats; /* 48 bytes */
int rt_frame_open_ex(rt_ctx* ctx, const rt_camera* cam, const rt_render_params* p, uint32_t frame_flags,
                     rt_frame** out);
int rt_frame_moments(rt_frame* f, double* out_q);
int rt_frame_restore_ex(rt_ctx* ctx, const void* buf, size_t len, const double* moments, rt_frame** out);
int rt_frame_error(rt_frame* f, const rt_error_tol* tol, double* out_se, rt_error_stats* out);
int rt_error_estimate(const double* sums, const double* moments, int64_t pixels, int chunks_done,
                      int samples_done, const rt_error_tol* tol, double* out_se, rt_error_stats* out);
#define RT_ADAPT_NAN 1u       /* stop pixels whose running sum has a NaN channel (frame_resolve's nan_pixels) */
#define RT_ADAPT_CONVERGED 2u /* stop finite pixels converged under (abs_tol, rel_tol), rt_frame_error's rule */
typedef struct rt_adapt_rule {
    double abs_tol;
    double rel_tol;
    int32_t min_chunks;
    uint32_t flags;
} rt_adapt_rule; /* 24 bytes */
typedef struct rt_adapt_stats {
    int32_t chunks_done;
    int32_t _pad;
    int64_t pixels;
    int64_t active_pixels;
    int64_t stopped_nan;
    int64_t stopped_converged_or_masked;
    int64_t stopped_now;
} rt_adapt_stats; /* 48 bytes */
int rt_frame_adapt(rt_frame* f, const rt_adapt_rule* rule, rt_adapt_stats* out);
int rt_frame_stop(rt_frame* f, const uint8_t* mask, rt_adapt_stats* out);
int rt_frame_chunk_counts(rt_frame* f, int32_t* out_chunks);
int rt_adapt_decide(const double* sums, const double* moments, const int32_t* chunks_in, int64_t pixels,
                    int chunks_done, int chunk, int spp, const rt_adapt_rule* rule, int32_t* chunks_out,
                    rt_adapt_stats* out);
/* Shard frames (above). The d_* pointers are device memory on the frame's device. */
int rt_frame_open_shard(rt_ctx* ctx, const rt_camera* cam, const rt_render_params* p, uint32_t frame_flags,
                        rt_frame** out);
int rt_frame_resolve_shard(rt_frame* f, uint8_t* d_slab_rgb8, double* d_slab_linear, rt_frame_stats* out);
int rt_frame_error_shard(rt_frame* f, const rt_error_tol* tol, double* d_slab_se, rt_error_stats* out);
int rt_error_stats_merge(const rt_error_stats* parts, int n, rt_error_stats* out);
int rt_frame_shard_state(rt_frame* f, double* d_slab_sums, double* d_slab_moments, int32_t* d_slab_chunks);
int rt_frame_save_header(rt_frame* f, void* buf, size_t cap);
int rt_frame_restore_shard(rt_ctx* ctx, const void* buf, size_t len, const double* moments, int shard_rank,
                           int shard_count, rt_frame** out);
/* Checkpoints (above): the version-2 blob. */
typedef struct rt_frame_ckpt_desc {
    rt_frame_blob_desc blob; /* version 1 or 2; payload_bytes = the bytes after the blob's own header */
    uint32_t sections;
    uint32_t _pad;
    uint64_t sums_offset;
    uint64_t moments_offset; /* 0: no Q */
    uint64_t stops_offset;   /* 0: no K */
    int64_t stopped_pixels;
    int64_t stopped_nan;
    int64_t active_pixels;
} rt_frame_ckpt_desc; /* 344 bytes */
int rt_frame_checkpoint_info(const void* buf, size_t len, rt_frame_ckpt_desc* out);
int rt_checkpoint_resolve(const void* buf, size_t len, uint8_t* out_rgb8, double* out_linear, rt_frame_stats* out);
int rt_checkpoint_error(const void* buf, size_t len, const rt_error_tol* tol, double* out_se, rt_error_stats* out);
int rt_frame_checkpoint(rt_frame* f, void* buf, size_t cap, size_t* out_len);
int rt_frame_resume(rt_ctx* ctx, const void* buf, size_t len, rt_frame** out);
int rt_frame_resume_shard(rt_ctx* ctx, const void* buf, size_t len, int shard_rank, int shard_count,
                          rt_frame** out);
int rt_frame_shard_stops(rt_frame* f, int32_t* d_slab_stops);
int rt_frame_checkpoint_header(rt_frame* f, uint32_t sections, int chunks_done, void* buf, size_t cap);
/* The fingerprint rt_upload_scene records for a descriptor (host only; the blob's field at 272). */
int rt_scene_fingerprint(const rt_scene_desc* desc, uint64_t* out);
/* The chunking of a tier-B frame of `pixels` pixels at `spp` samples (host only): *out_chunk =
 * rt_sample_chunk(pixels, spp), *out_chunks_total = ceil(spp / chunk). For callers that cannot use the
 * header's inline (other languages): one rule, this header's. */
int rt_frame_chunking(int64_t pixels, int spp, int* out_chunk, int* out_chunks_total);
/* The denoised preview of an unsharded frame (the feature-guided denoiser, above). */
int rt_frame_denoise(rt_frame* f, const rt_denoise_params* params, const double* d_feature_sums, uint8_t* out_rgb8,
                     double* out_linear, rt_denoise_stats* stats);

/*
 * Debug / parity entry: closest hit of n world rays (7 doubles each: origin, direction, time)
 * in [tmin, tmax]. out: 12 doubles per ray: hit(0/1), t, p xyz, normal xyz, u, v, front_face,
 * material. Media draws use tier-B stream (seed, pixel_id = ray index, sample 0).
 * flags: RT_FLAG_REFERENCE_CULL as for rendering, plus one walk selector: none = the recursive
 * walk (media and frames allowed); RT_DEBUG_RESUMABLE = the render loop's resumable binary
 * walk (media and frames in the reference's order, frames nesting at most RT_MAX_FRAMES deep, else
 * RT_E_UNSUPPORTED); RT_DEBUG_WIDE = the resumable walk over the 4-wide fp32-box tree, which, like
 * RT_DEBUG_QNODE, needs a world without ConstantMedium and instance frames (else RT_E_UNSUPPORTED,
 * checked before anything is allocated or launched).
 */
#define RT_DEBUG_RESUMABLE 4u
#define RT_DEBUG_WIDE 8u
#define RT_DEBUG_QNODE 16u /* the 4-wide walk over the quantised tree (rt_qnode) and sphere quadruples that the
                              global-memory kernels of spheres-only worlds take */
int rt_debug_closest_hits(rt_ctx* ctx, const double* rays, int n, double tmin, double tmax,
                          uint64_t seed, uint32_t flags, double* out);
/*
 * Debug: how the 4-wide walk orders a node's children (include/rt_wide.h, packed sort keys). out[0] = 1 when
 * the ctx's last tier-B launch, or its last rt_debug_closest_hits call with RT_DEBUG_WIDE if that came later,
 * sorted packed keys (0: key / reference pairs, or no 4-wide walk); out[1] = 1 when the uploaded world's
 * 4-wide tree is within the packed keys' id bound; out[2] = the bits a packed word gives the child
 * reference; out[3] = the most 4-wide nodes an LDS-staged launch can be given (every such tree is within
 * the bound). Either form computes the same hits and images.
 */
int rt_debug_wide_keys(rt_ctx* ctx, int out[4]);

/*
 * Debug / parity entry: single hot-path functions on the device (golden vectors per function,
 * tests/golden/make_function_goldens.py). Record i draws from its own tier-B Philox stream
 * (key = seed, pid = i, sample 0). Layouts (doubles per record), in -> out:
 *   RT_PROBE_SCATTER      scatter (src/Lib.hs:822-865; emitted 880-885 for DiffuseLight):
 *                         ray o3 d3 tm, hit t p3 n3 u v front_face material (18) ->
 *                         scattered (0/1), ray o3 d3 tm, att3 (the emission when not scattered),
 *                         pdf, specular, Philox words consumed (14)
 *   RT_PROBE_HTBL_RANDOM  htblRandom on the lights tree (src/Lib.hs:707-724): origin3 -> dir3, words
 *   RT_PROBE_HTBL_PDF     htblPdfValue on the lights tree (src/Lib.hs:673-705): origin3, v3 -> pdf, words
 *   RT_PROBE_TEXTURE      textureValue (src/Lib.hs:496-513): texture id, u, v, p3 -> albedo3
 *   RT_PROBE_GET_RAY      getRay with `cam` (src/Lib.hs:1253-1267): s, t -> ray o3 d3 tm, words
 *   RT_PROBE_BOX          the BVH box test: box min3 max3, ray o3 d3, t_min, t_max (14) -> the default test
 *                         as the walks run it (division-free, rt_trace.h box_hit), the same test with
 *                         divisions, the reference's per-axis boxRayIntersect (src/Lib.hs:798-814) (3; 1 = hit)
 */
/*
 * Debug / parity entry: tier A (RT_RNG_EXACT) over the whole frame, with column `col`'s path segments
 * recorded: 10 doubles per segment {row, sample (in the order rendered), seg (or -(seg + 1) where the
 * path ends), the scattered ray's origin xyz and direction xyz (at the end: the segment's own ray), the
 * column generator's seed after the segment (the uint64 bits)}. *out_n = segments recorded (at most
 * cap). The oracle's oracle_exact_trace records the same, so the first differing record localises a
 * tier-A divergence.
 */
int rt_debug_exact_trace(rt_ctx* ctx, const rt_camera* cam, const rt_render_params* p, const uint64_t* col_gens,
                         int col, double* out, int cap, int* out_n);

#define RT_PROBE_SCATTER 0
#define RT_PROBE_HTBL_RANDOM 1
#define RT_PROBE_HTBL_PDF 2
#define RT_PROBE_TEXTURE 3
#define RT_PROBE_GET_RAY 4
#define RT_PROBE_BOX 5
int rt_debug_probe(rt_ctx* ctx, const rt_camera* cam, int op, const double* in, int n, uint64_t seed, double* out);

/*
 * Debug / numerics probe: out[i] = op(x[i], y[i]) evaluated on the device.
 * ops: 0 x/y (IEEE), 1 div_exact(x, y) (reciprocal + Markstein), 2 sqrt x, 3 sin x, 4 cos x,
 * 5 atan x, 6 asin x, 7 log x, 8 pow(x, y), 9 GHC atan2(x, y), 10 tan x, 11 the render path's
 * x ** 5 (schlick; double-double, correctly rounded); 12-16 include/rt_libm.h's sin, cos, atan, asin,
 * log x and 17 GHC atan2(x, y) over them (RT_FLAG_SHARED_LIBM); 18 and 19 the sine and the cosine of x from
 * the sincos call of the kernels that fuse the two.
 */
int rt_debug_math(rt_ctx* ctx, int op, const double* x, const double* y, int n, double* out);

#ifdef __cplusplus
}
#endif
#endif /* RT_H */
