/* pt_api.h -- C ABI of the MI355X path-tracing hot path (HIP kernels for gfx950).
 *
 * Drop-in for the reference's GL compute-program interface:
 *   ComputeShader("computeShader.c")                 shader_c.h:14-60          -> pt_create
 *   SSBOs at bindings 4..8 (glMapBufferRange)        ogl_path_trace.h:383-529  -> pt_upload_scene
 *   camera SSBO re-upload (glBufferData)             ogl_path_trace.h:322-326  -> pt_set_camera
 *   setInt("frame"/"accumulate"/"displayMode"...)    ogl_path_trace.h:174-182  -> pt_render args
 *   glDispatchCompute(W/10, H/10, 1)                 ogl_path_trace.h:183      -> pt_render
 *   glMemoryBarrier + textured quad readback         ogl_path_trace.h:186-192  -> pt_read_rgba32f
 *   ACESFilm fragment shader                         screenQuadFrag.c:12-33    -> pt_read_rgba8_aces
 *
 * No torch / C++ types cross this boundary.  Every call is synchronous w.r.t. the host
 * unless named *_async.  A context is not thread-safe: one context per thread.
 * Return 0 on success, a negative PT_E* code otherwise; pt_last_error() explains.
 */
#ifndef PT_API_H
#define PT_API_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PT_OK 0
#define PT_E_ARG (-1)      /* bad argument / size */
#define PT_E_IO (-2)       /* file could not be opened */
#define PT_E_PARSE (-3)    /* OBJ/MTL line too long or malformed */
#define PT_E_SCENE (-4)    /* scene violates a limit or layout assumption */
#define PT_E_HIP (-5)      /* HIP runtime error (no device, OOM, launch failure) */
#define PT_E_STATE (-6)    /* call out of order (e.g. render before upload) */

/* Flags mirroring the shader's compile-time toggles (computeShader.c:77-82). */
#define PT_FLAG_NO_AA 1          /* antiAlias = false */
#define PT_FLAG_NO_SKY 2         /* EnvironmentEnabled = false */
#define PT_FLAG_NO_SPHERES 4     /* render_spheres = false */
#define PT_FLAG_NO_TRIANGLES 8   /* render_triangles = false */
#define PT_FLAG_REF_DISPATCH 16  /* write only the 10x10-group footprint of
                                    glDispatchCompute(W/10, H/10) (ogl_path_trace.h:183) */
#define PT_FLAG_MOLLER_TRUMBORE 32 /* opt-in fast mode: the reference's (dead) Moller-Trumbore
                                    RayIntersectsTriangle (computeShader.c:228-272) replaces the
                                    live hit_triangle (:274-307).  NOT the reference's image:
                                    pixels differ where the two tests disagree (tolerance in
                                    tests/test_gpu_parity.py); bit-exact to the oracle's MT mode */
#define PT_FLAG_ALL 63

typedef struct pt_ctx pt_ctx;

typedef struct {
    int width, height;       /* framebuffer (TEXTURE_WIDTH/HEIGHT, ogl_path_trace.h:45-46) */
    int max_bounce;          /* maxBounceCount; loop is i <= max_bounce (computeShader.c:74,447) */
    int display_mode;        /* 1 shaded, 2 normals, 3 albedo, 4 distance (computeShader.c:454-481) */
    int flags;               /* PT_FLAG_* */
    int rays_per_pixel;      /* raysPerPixel (computeShader.c:507); 1 in the reference */
    int device;              /* HIP device ordinal */
    int rank, world;         /* image partition: this context owns rows y = rank + k*world */
} pt_config;

int pt_create(const pt_config* cfg, pt_ctx** out);
void pt_destroy(pt_ctx* ctx);
const char* pt_last_error(const pt_ctx* ctx);

/* Scene upload in the reference's std140 layouts (see pt_scene.h).  The library validates
 * links/indices and transposes to its device layouts. */
int pt_upload_scene(pt_ctx* ctx, const float* tris, int n_tris, const float* bvh, int n_nodes,
                    const float* mats, int n_mats, const float* spheres, int n_spheres);

/* cam: 12 floats {position.xyzw, direction.xyzw, data.xyzw} (computeShader.c:50-55). */
int pt_set_camera(pt_ctx* ctx, const float cam[12]);
/* Uniform displayMode (1..4), set per frame by the reference (ogl_path_trace.h:182; the
 * keys 1-4 change it, :261-265).  Replaces pt_config.display_mode for later renders. */
int pt_set_display_mode(pt_ctx* ctx, int display_mode);

/* Equivalent to n_frames reference dispatches with frame = frame_first .. frame_first+n-1;
 * only the first uses accumulate = accumulate_first, the rest accumulate = 1 (running
 * mean, computeShader.c:548-551).  Bit-identical to n_frames separate calls, for any
 * n_frames: a render too large for one launch's scratch is split (tuning key 8). */
int pt_render(pt_ctx* ctx, int frame_first, int n_frames, int accumulate_first);
/* Same, enqueued on the context's stream without waiting (timing / overlap). */
int pt_render_async(pt_ctx* ctx, int frame_first, int n_frames, int accumulate_first);
int pt_sync(pt_ctx* ctx);

/* Progressive rendering as a replayed hipGraph (the reference's endless render loop,
 * ogl_path_trace.h:160-204, without a host round trip per frame): setup captures
 * `launches_per_replay` launches of `frames_per_launch` frames each plus a device-side
 * frame-counter advance; every replay renders the next frames_per_launch*launches frames.
 * Frame 1 is rendered with accumulate = 0 (a reset), later frames accumulate.  reset()
 * sets the next frame number (1 = restart accumulation).  The graph is dropped whenever
 * the scene, camera, kernel or tuning changes.  run() is asynchronous (pt_sync waits). */
int pt_progressive_setup(pt_ctx* ctx, int frames_per_launch, int launches_per_replay);
int pt_progressive_reset(pt_ctx* ctx, int next_frame);
int pt_progressive_run(pt_ctx* ctx, int replays);

/* Local rows owned by this context: rows y = rank + k*world, k < rows_local. */
int pt_rows(const pt_ctx* ctx, int* rows_local, int* row0, int* row_stride);
/* The context's configuration as created (display_mode as last set). */
int pt_get_config(const pt_ctx* ctx, pt_config* out);

/* Copies the local accumulation rows (rows_local * width * 4 floats, local row 0 =
 * image row `rank`, image row 0 = bottom). */
int pt_read_rgba32f(pt_ctx* ctx, float* host_dst, size_t bytes);
/* ACES-tonemapped RGBA8 of the local rows, computed on the device. */
int pt_read_rgba8_aces(pt_ctx* ctx, unsigned char* host_dst, size_t bytes);
/* Asynchronous presentation, for a loop that shows every frame (the reference draws each
 * frame's texture, ogl_path_trace.h:189-192).  pt_present_begin(buf) enqueues the ACES
 * epilogue of the image as of the renders issued so far, and its copy into the context's
 * pinned host buffer `buf` (0..3), both on the context stream; it does not wait, and later
 * renders overlap the copy.  When the caller presented after its previous render too, the
 * latest render's accumulate pass already wrote the view and only the copy is enqueued (a
 * write through pt_accum_device's pointer or onto pt_stream's stream must therefore come
 * after those calls, not before with a pointer kept from earlier).
 * pt_present_end(buf) waits for that copy and returns the
 * rows_local * width RGBA8 pixels (same bytes as pt_read_rgba8_aces), valid until the next
 * pt_present_begin on `buf` or pt_destroy.  Showing frame f-2 while frames f-1 and f render
 * (three buffers in rotation) keeps renders in flight, as the render-only loop does.
 * A buffer begun again before its end first waits for its previous copy.
 * PT_E_STATE: end without a begin. */
int pt_present_begin(pt_ctx* ctx, int buf);
int pt_present_end(pt_ctx* ctx, int buf, const unsigned char** pixels);
/* Overwrites the local accumulation rows (resume from a checkpoint / seed a test). */
int pt_write_rgba32f(pt_ctx* ctx, const float* host_src, size_t bytes);

/* Device pointer + size of the local accumulation buffer (for RCCL gathers). */
int pt_accum_device(pt_ctx* ctx, void** dev_ptr, size_t* bytes);
/* Stream-ordered device-to-device copy of the local rows into caller device memory
 * (e.g. an RCCL send buffer); returns after the copy completed. */
int pt_copy_rows_device(pt_ctx* ctx, void* dst_dev, size_t bytes);
/* The hipStream_t the context renders on (as void*). */
int pt_stream(pt_ctx* ctx, void** stream);

/* Statistics of the last pt_render*: kernel ms (HIP events on the render stream), and
 * when counting is enabled the reference-semantics work counts:
 * out[0] segments, [1] node visits, [2] triangle tests, [3] sphere tests, [4] hits. */
int pt_set_counting(pt_ctx* ctx, int enable);
int pt_stats(pt_ctx* ctx, double* kernel_ms, unsigned long long out[5]);
/* Counting-build diagnostics of the last render: out[0..4] as pt_stats, then per kernel
 * phase (traversal step, leaf test, segment) the wave iterations and the active lanes
 * summed over them: [5] trav waves, [6] trav lanes, [7] leaf waves, [8] leaf lanes,
 * [9] segment waves, [10] segment lanes (persistent kernels; 0 for the tiled kernel),
 * [11] segments outside the exact-reciprocal guard (state-machine kernel), [12] segments
 * that met a NaN.  Scene facts (any build): [13] bytes of the LDS scene copy, [14] the same
 * with the culling walk's sink image (0 when the tree does not qualify); [15] 1 when the
 * uploaded tree qualifies for the culling walk, it is on (tuning key 15) and the sink image
 * costs no resident workgroup per CU at the set waves per SIMD (key 3), else 0. */
int pt_stats_ex(pt_ctx* ctx, unsigned long long out[16]);
/* Render-kernel launches this context has enqueued since pt_create: out[0] on a generic line,
 * out[1] on the specialised default-path line (tuning key 21).  A captured progressive graph
 * counts once, at capture; its replays run the line it was captured with. */
int pt_debug_launches(pt_ctx* ctx, unsigned long long out[2]);
/* The window clause of the LDS culling walk (tuning key 22): *active = 1 when the context's
 * LDS launches run it (the walk culls, the key leaves it on, no Moller-Trumbore, every
 * triangle of the scene inside the clause's conditions), *slack = the uploaded scene's window
 * slack (the largest of its three axes; 0 for a scene outside the conditions).  Either
 * pointer may be null. */
int pt_debug_window_cull(pt_ctx* ctx, int* active, float* slack);
/* The leaf sweep (tuning key 23): *swept = 1 when the render launch this context enqueued last
 * ran it, *qualifies = 1 when the uploaded scene has a sweep table, *n_leaves = the scene's leaf
 * pairs.  Any pointer may be null. */
int pt_debug_sweep(pt_ctx* ctx, int* swept, int* qualifies, int* n_leaves);
/* The path pool (tuning key 24): *pooled = 1 when the render launch this context enqueued last
 * ran the pool kernel of the specialised swept line.  The pointer may be null. */
int pt_debug_pool(pt_ctx* ctx, int* pooled);
/* The adaptive tile order (tuning key 2), read only: waits for the context's work, then
 * *sorts = the tile-order sorts run since the last scene upload (a captured graph's sorts count
 * once per replay), *n_tiles and *tiles_x = the work queue's tile grid (tuning key 20), and
 * perm_out[0 .. *n_tiles) = the order the next launch reads, one (ty << 16) | tx per tile
 * (PT_E_ARG when max_tiles is smaller than the grid).  Any pointer may be null.  Changes no
 * launch. */
int pt_debug_tile_order(pt_ctx* ctx, unsigned long long* sorts, unsigned* perm_out, int max_tiles, int* n_tiles,
                        int* tiles_x);
/* Sum of render-kernel durations (HIP events on the render stream) and the number of
 * launches since the last reset; reset != 0 clears both after reading. */
int pt_timing(pt_ctx* ctx, double* total_kernel_ms, int* n_launches, int reset);

/* Kernel variant selection: 0 = the state-machine kernel (default), 3 = the same kernel with
 * the scene kept in global memory even when it would fit LDS (A/B of the LDS staging). */
int pt_set_kernel(pt_ctx* ctx, int variant);
/* Scheduling knobs of the state-machine kernel:
 * key 0 = run the leaf phase once this many lanes wait at leaves (1..64, 0 = auto),
 * key 1 = run the shading phase once this many lanes finished their segment (1..64, 0 = auto),
 * key 2 = adaptive tile order (1 default: 8x8 tiles are queued most-expensive-first using
 *         the segment counts of the previous renders; 0 = raster order),
 * key 3 = resident waves per SIMD the kernel is compiled for (5..8; 0 = auto: 7 for scenes
 *         staged in LDS, 6 for global-memory scenes),
 * key 4 = queue ids a wave reserves per queue atomic in frame-split mode (1..1024; 0 = auto:
 *         256 / 64 for LDS-staged scenes with items of 1 / 2 frames, else about the launch's
 *         queue ids per resident wave / (8 x frames per item), clamped to 32..256).
 * key 5 = frames per work item (>= 1; 0 = auto, 2..8): a pixel's frames are spread over
 *         several lanes and the running mean is applied by a second kernel in frame order;
 *         a value >= n_frames gives each lane whole pixels (running mean in registers).
 *         In automatic mode launches of at most 16 frames always take the split path (its
 *         batched queue reservations), whatever their group.  While the moments are on
 *         (pt_set_moments) every launch takes the split path, since the accumulate pass keeps
 *         them: a value >= n_frames then means one item per pixel, still split.
 * key 6 = walk floor (1..64, 0 = auto): a walk phase ends once fewer lanes than this still
 *         walk, and the leaf (or shading) phase runs even below its threshold.
 * key 7 = leaf-phase compaction limit (0..63, default 63): the edge tests of a wave's leaf
 *         phase are packed onto its first lanes when at most this many (lane, triangle) pairs
 *         need them; 0 = every lane tests its own triangles.
 * key 8 = frame-split scratch budget in MiB (0 = automatic: min(32 GiB, device memory / 4)).
 *         A render whose per-frame colours (12 B per pixel-frame) exceed it -- or whose
 *         32-bit work-queue ids would overflow -- runs as back-to-back launches, the first
 *         with the caller's accumulate flag and the rest accumulating: the same image.
 * key 9 = overlapped short launches: render slots 2..4, 1 = off, 0 = automatic (3).  Renders
 *         of at most 16 frames (the reference's one dispatch per displayed frame) run their
 *         render kernel on one of these extra streams, so the next render fills the CUs that
 *         this one's launch tail frees; the running mean is still applied on the context's
 *         stream in frame order.
 * key 15 = culling walk (0 = automatic, 1 = off).  When the uploaded tree is a full binary
 *         tree threaded in preorder whose internal boxes contain their children's, the
 *         LDS-staged walk tests nodes with a cheaper conservative slab test and re-tests a
 *         leaf's box exactly before one of its triangles may move t.
 * key 16 = wide global-memory walk (0 = automatic, 1 = off: the binary walk).  Scenes too
 *         large for LDS with a nested tree walk a 4-wide tree of quantised child boxes
 *         (DESIGN.md §5.10).
 * key 17 = threads per workgroup of the wide walk: 256, 512, 768 or 1024 (0 = automatic, 256).
 * key 18 = overlapped short renders: 256-thread blocks per CU, 1..8 (0 = automatic: 3 with
 *         three or more render slots, 5 when the caller presents every frame).
 * key 19 = leaf re-test certificate (0 = automatic, 1 = off).  The wide walk skips the exact
 *         leaf-box re-test for a hit whose triangle data proves it passes;
 *         only for uploaded trees whose leaf boxes contain their triangles' vertices.
 * key 20 = work-queue tile shape: 1 = 8x8, 2 = 16x4, 3 = 32x2, 4 = 64x1 pixels (columns x local
 *         rows), 0 = automatic (8x8).  A change drains the context's streams and
 *         drops a captured graph.
 * key 21 = specialised default-path kernel (0 = automatic, 1 = off: always the generic kernel).
 *         A frame-split launch of the default configuration -- shaded mode, no flags, one ray
 *         per pixel, one sphere, a scene staged in LDS with the culling walk, 8x8 tiles in a
 *         learned order, automatic thresholds and occupancy -- runs a build of the kernel that
 *         holds these launch-wide facts as constants; every other launch, and
 *         a context's launches before its first tile-order sort, run the generic one.
 * key 22 = window clause of the LDS culling walk (0 = automatic, 1 = off).  The walk skips a
 *         box that ends before the distance window (1e-4, t) in which a triangle can be
 *         accepted; off, launches run the generic kernel without the clause.
 * key 23 = leaf sweep (0 = automatic, 1 = off: the culling walk).  In a scene of a few leaves
 *         a ray inside the exact-reciprocal guard tests every leaf box once per segment, with
 *         bounds that are the same for all lanes, instead of walking the tree ("The leaf sweep").
 * key 24 = path pool (0 = automatic, 1 = off).  Launches of the specialised swept line that run on the
 *         context's own stream (every launch but an overlapped short one, key 9) keep the path
 *         state in a per-wave LDS pool and hand any path to any lane.
 * None of these change the image (each pixel's frames stay in order in one lane). */
int pt_set_tuning(pt_ctx* ctx, int key, int value);

/* Per-pixel noise estimate and render-until-converged.
 *
 * With moments on, the accumulate pass keeps two sums per local pixel beside the image: for
 * each frame's colour c, in frame order, as separately rounded binary32 operations,
 *   Y = (c.x*0.2126f + c.y*0.7152f) + c.z*0.0722f;   S1 = S1 + Y;   S2 = S2 + Y*Y;
 * They restart from (0, 0) whenever the image does (a render with accumulate = 0, frame 1 of
 * a progressive run) and continue otherwise; pixels outside the dispatch footprint
 * (PT_FLAG_REF_DISPATCH) are never touched.  `frames` is the number n of frames folded in
 * since that restart.  The relative error of a pixel after n >= 2 frames, nf = (float)n:
 *   m = S1/nf;  v = max(S2/nf - m*m, 0);  sem = sqrt(v/(float)(n-1));  rel = sem/(m + 0.01f);
 *   rel = 64 unless 0 <= rel <= 64 (NaN or infinite moments included);
 *   q = (unsigned)(rel * 65536.0f)                   (truncated; q <= 2^22)
 * The summary holds integers only, so it does not depend on the order of the reduction and
 * adds exactly across the contexts of a split image (pt_group_noise). */
typedef struct {
    unsigned long long pixels;   /* footprint pixels of the local rows */
    unsigned long long sum_q;    /* sum of q  (mean rel = sum_q / pixels / 65536) */
    unsigned long long above;    /* pixels with q > (unsigned)(target * 65536.0f) */
    unsigned int max_q;
    int frames;                  /* n */
} pt_noise_stats;

/* Turns the moments on (allocated and zeroed) or off (freed); frames = 0 either way.  While
 * they are on every launch runs in frame-split mode (tuning key 5); the image is the same
 * with them on or off.  A change drains the context's streams and drops a captured graph.
 * pt_write_rgba32f, pt_set_camera and pt_upload_scene leave the moments alone: the caller's
 * next restarting render clears them, as it does the image. */
int pt_set_moments(pt_ctx* ctx, int enable);
/* The local rows' moments, rows_local * width * 2 floats (S1, S2 per pixel, pixel order of
 * pt_read_rgba32f), and the frames in them.  PT_E_STATE: moments off. */
int pt_read_moments(pt_ctx* ctx, float* host_dst, size_t bytes, int* frames);
/* The summary of the local rows, reduced on the device.  PT_E_STATE: moments off or fewer
 * than 2 frames. */
int pt_noise(pt_ctx* ctx, float target, pt_noise_stats* out);
/* The same summary on the host, of n_pixels moment pairs; in_footprint (may be NULL = all)
 * holds one byte per pixel, 0 = outside the footprint.  No device is touched: the per-pixel
 * function is the device kernel's own code.  PT_E_ARG: frames < 2 or a null pointer. */
int pt_noise_host(const float* moments, const unsigned char* in_footprint, size_t n_pixels, int frames,
                  float target, pt_noise_stats* out);
/* Renders frames frame_first, frame_first + 1, ... `batch` at a time (the first batch with
 * the caller's accumulate flag, the rest accumulating) and stops after the first batch whose
 * mean relative error is at or below `target`, sum_q <= (unsigned)(target * 65536.0f) *
 * pixels, or after max_frames frames (the last batch may be shorter).  Turns the moments on
 * if they are off.  Synchronous: one host round trip per batch.  The image afterwards is
 * that of pt_render(frame_first, *frames_done, accumulate_first), bit for bit; `last` (may be
 * NULL) receives the final summary.  PT_E_ARG: batch < 2, max_frames < batch or target <= 0. */
int pt_render_until(pt_ctx* ctx, int frame_first, int accumulate_first, int batch, int max_frames,
                    float target, int* frames_done, pt_noise_stats* last);

/* Adaptive sampling: pt_render_until's batches, but every tile of the work
 * queue stops on its own.  The unit is the queue's tile, (8 << s) columns x (8 >> s) local rows
 * (tuning key 20), numbered ty * tiles_x + tx as in pt_debug_tile_order; a row-split context
 * decides on its own local tiles.  Frames frame_first, frame_first + 1, ... are rendered `batch`
 * at a time (the last batch may be shorter) for the tiles still active, and for no other tile.
 * After a batch, with n = n0 + the frames done so far (n0 = 0 for a restarting call, the
 * context's frame count for accumulate_first = 1), an active tile retires when the sum of q =
 * quantise(S1, S2, n) over its footprint pixels is at most (unsigned)(target * 65536.0f) times
 * their number.  A retired tile is frozen: the call neither reads nor writes its image pixels
 * and moments again, so a pixel holds the image and the moments of pt_render(frame_first, f,
 * accumulate_first), bit for bit, f being the frames its tile received.  A tile without a
 * footprint pixel (outside PT_FLAG_REF_DISPATCH's footprint, beyond the local rows) is never
 * active and has f = 0.  The call ends when no tile is active or after max_frames frames;
 * *frames_done = the frames the longest-lived tile received in this call.  Turns the moments on
 * if they are off.  Synchronous: one host round trip per batch.
 *
 * Afterwards the moments hold per-tile frame counts: pt_read_moments reports the largest, and
 * pt_noise, pt_render_until, pt_group_noise and a further pt_render_adaptive with
 * accumulate_first = 1 return PT_E_STATE until a restarting render (accumulate = 0) or
 * pt_set_moments makes the counts uniform again.  Plain renders are allowed at any time and
 * behave as ever.  The contexts of a pt_group are not coordinated: group support is out of
 * scope, each context of a group would stop its tiles alone.
 * PT_E_ARG: batch < 2, max_frames < batch or target <= 0.  PT_E_STATE: before an upload. */
typedef struct {
    pt_noise_stats noise;              /* every footprint pixel quantised with its own tile's n;
                                          frames = the largest n */
    unsigned long long tiles;          /* tiles that hold a footprint pixel */
    unsigned long long tiles_active;   /* ... of them, still above the target at the stop */
    unsigned long long pixel_frames;   /* sum over tiles of footprint pixels x f */
} pt_adaptive_stats;
int pt_render_adaptive(pt_ctx* ctx, int frame_first, int accumulate_first, int batch, int max_frames,
                       float target, int* frames_done, pt_adaptive_stats* last);
/* The frames f each tile received in the last pt_render_adaptive: waits for the context's work,
 * then *n_tiles and *tiles_x = the tile grid and dst[0 .. *n_tiles) = f per tile (PT_E_ARG when
 * max_tiles is smaller than the grid; all 0 before the first adaptive call).  Any pointer may
 * be null. */
int pt_read_tile_frames(pt_ctx* ctx, unsigned* dst, int max_tiles, int* n_tiles, int* tiles_x);
/* The stop rule on the host, of one tile's n_pixels moment pairs (in_footprint as in
 * pt_noise_host): *retires = 1 when the tile would retire after `frames` frames.  No device is
 * touched: the rule is the device kernel's own code.  PT_E_ARG as pt_noise_host. */
int pt_tile_retires_host(const float* moments, const unsigned char* in_footprint, size_t n_pixels, int frames,
                         float target, int* retires);

/* Denoised view: an edge-avoiding a-trous filter of the accumulation image, guided
 * by first-hit normal, albedo and distance and, with moments of n >= 2 frames, by the per-pixel
 * variance of the mean luminance (after pt_render_adaptive: with each tile's own frame count).
 * A view only: the image, the moments and every launch stay what they are without it.
 *
 * iterations 1..8 (iteration i takes its 5x5 taps 1 << i pixels apart), guide_frames >= 1 (frames
 * averaged into the guides), and one sigma per factor; a NaN or non-positive sigma switches its
 * factor off.  Defaults: 5, 4, and 8 / 0.1 / 0.1 / 0.05. */
typedef struct {
    int iterations;
    int guide_frames;
    float sigma_lum, sigma_normal, sigma_albedo, sigma_depth;
} pt_denoise_params;
void pt_denoise_defaults(pt_denoise_params* params);
typedef struct {
    int guided;            /* 1: the luminance factor ran (moments on, n >= 2 frames) */
    int guides_rendered;   /* 1: this call rendered the guides, 0: it found them cached */
    int iterations;
    int frames;            /* n of the moments (the largest after an adaptive run), 0 when they are off */
} pt_denoise_info;
/* Filters the image as of the renders issued so far, on the context stream behind their
 * accumulate passes (as pt_present_begin), and waits.  params NULL = the defaults; info may be
 * NULL.  The guides are the images pt_render(1, guide_frames, 0) would produce in display modes
 * 2, 3 and 4 with the context's scene, camera, flags and rays per pixel; they are rendered by the
 * first call and kept until pt_upload_scene, pt_set_camera or another guide_frames.  Pixels
 * outside the dispatch footprint (PT_FLAG_REF_DISPATCH) are copied through.
 * PT_E_STATE: before an upload, or on a row-split context (world > 1: its interleaved rows have
 * no neighbours; denoising a pt_group is out of scope).  PT_E_ARG: iterations or guide_frames
 * out of range. */
int pt_denoise(pt_ctx* ctx, const pt_denoise_params* params, pt_denoise_info* info);
/* Same, enqueued without waiting (pt_sync, or a read below, waits). */
int pt_denoise_async(pt_ctx* ctx, const pt_denoise_params* params, pt_denoise_info* info);
/* The last denoise's result: width * height * 4 floats, rgb filtered, alpha the image's.
 * PT_E_STATE: no denoise yet. */
int pt_read_denoised_rgba32f(pt_ctx* ctx, float* host_dst, size_t bytes);
/* ... and its ACES-tonemapped RGBA8, computed on the device (as pt_read_rgba8_aces). */
int pt_read_denoised_rgba8_aces(pt_ctx* ctx, unsigned char* host_dst, size_t bytes);
/* The guides of the last denoise, 8 floats per pixel: N.rgb, Z, A.rgb, 0.  PT_E_STATE: no denoise yet. */
int pt_read_guides(pt_ctx* ctx, float* host_dst, size_t bytes);
/* The filter on the host: image W*H*4 floats, variance W*H floats of the mean luminance's
 * variance (NULL = unguided), guides W*H*8 floats as pt_read_guides, in_footprint one byte per
 * pixel (NULL = all), out W*H*4 floats.  No device is touched: the per-tap code is the device
 * kernel's own.  PT_E_ARG: a null pointer, a size <= 0 or parameters out of range. */
int pt_denoise_host(const float* image, const float* variance, const float* guides, const unsigned char* in_footprint,
                    int W, int H, const pt_denoise_params* params, float* out);

/* Ray queries: what a caller's ray hits in the uploaded scene -- picking, focus distance, visibility
 * and occlusion probes, collision -- on the resident BVH and with the render's bit-exact walk.
 *
 * The result of a ray is the reference's calculateRayCollision (computeShader.c:367-432) with t starting at t_max
 * instead of 1./0.: the spheres in index order, accepting 1e-4 < t_s < t, then the link walk from node 0 with
 * bvh_intersect at the current t and the 2-way choice at every hit leaf.  d is used as given, not normalised.  The
 * context's PT_FLAG_NO_SPHERES, PT_FLAG_NO_TRIANGLES and PT_FLAG_MOLLER_TRUMBORE apply as in a render.  t_max = +inf
 * is exactly the reference; a NaN or too-small t_max, NaN or zero ray components and an origin inside a sphere get no
 * special case and fall out of the IEEE arithmetic as they do there.  With PT_QUERY_ANY_HIT (occlusion) the ray stops
 * at the first acceptance in that same order and reports it: deterministic too.
 *
 * A query is invisible to rendering: it takes no timing events, touches no launch counter, tile order, moments,
 * presented state or captured graph, and writes nothing a render reads. */
typedef struct {
    float o[3];
    float t_max;
    float d[3];
    float pad;               /* 0 */
} pt_ray;                    /* 32 B */
#define PT_HIT_NONE 0
#define PT_HIT_SPHERE 1
#define PT_HIT_TRIANGLE 2
typedef struct {
    float t;                 /* +inf for a miss */
    int kind;                /* PT_HIT_* */
    int prim;                /* the sphere index, or the triangle index of the uploaded array (the leaf's data[0] /
                                data[1] that won); -1 for a miss */
    int mat;                 /* the material index; -1 for a miss */
    float n[4];              /* the reference's normal, flipped against d; n[3] = 0 */
    float p[4];              /* o + t*d, the multiply and the add rounded separately (hitPoint); p[3] = 0 */
} pt_hit;                    /* 48 B; a miss has n = p = 0 */
#define PT_QUERY_ANY_HIT 1
/* n rays from host arrays, synchronous.  PT_E_STATE before pt_upload_scene, PT_E_ARG for a null array with n > 0, a
 * negative n or unknown query flags; n = 0 is PT_OK without a launch.  A row-split context (world > 1) answers like
 * any other: every context holds the whole scene. */
int pt_intersect(pt_ctx* ctx, const pt_ray* rays, long long n, pt_hit* hits, int query_flags);
/* The same on device arrays (16-byte aligned), enqueued on the context's stream (pt_stream) behind the renders and
 * accumulate passes already enqueued, and not synchronised. */
int pt_intersect_device(pt_ctx* ctx, const void* d_rays, long long n, void* d_hits, int query_flags);
/* The camera rays of n pixels xy = {x0, y0, x1, y1, ...} (image row 0 = bottom) as a render with PT_FLAG_NO_AA
 * forms them: zero jitter, the camera basis as pt_set_camera derives it from cam, t_max = +inf.  Pure host code. */
int pt_pixel_rays(int width, int height, const float cam[12], const int* xy, long long n, pt_ray* rays_out);
/* pt_pixel_rays with the context's camera and size, then pt_intersect: what is under these pixels (a context
 * starts with the reference's default camera). */
int pt_pick(pt_ctx* ctx, const int* xy, long long n, pt_hit* hits);
/* The query on the host, of a scene in pt_upload_scene's arrays: packs it as pt_upload_scene does and runs the device
 * kernel's own per-ray code on the packed buffers.  No device is touched.  ctx_flags: the PT_FLAG_* a context would
 * hold.  Returns the packer's error for a rejected scene. */
int pt_intersect_host(const float* tris, int n_tris, const float* bvh, int n_nodes, const float* mats, int n_mats,
                      const float* spheres, int n_spheres, int ctx_flags, const pt_ray* rays, long long n,
                      pt_hit* hits, int query_flags);

/* Traced rays: the light that arrives along a caller's ray -- cameras the caller builds itself
 * (fisheye, stereo pairs), light probes and lightmap baking, the radiance behind a picked pixel, an integrator the
 * client drives itself.  A thin lens, orthographic views and anti-aliased panoramas are camera models (pt_trace_camera
 * below): a traced ray is the same in every frame of a call.
 *
 * For ray i and frame f the random state is seeds[i] + (uint32)f * 719393u, wrapping, and rgb is the reference's
 * Trace (computeShader.c:434-501) from o, d with that state: incoming light 0, ray colour 1, and for every segment up
 * to the context's max_bounce one closest hit as pt_intersect finds it, then the surface bounce, the sky or a
 * display-mode return as a render shades it.  d is used as given, not normalised; there are no jitter draws and no
 * rays_per_pixel: the ray is the caller's.  The first segment's search starts at the ray's t_max, later segments at
 * +inf; t_max = +inf is exactly the reference.  The context's max_bounce, display mode as last set, PT_FLAG_NO_SKY,
 * PT_FLAG_NO_SPHERES, PT_FLAG_NO_TRIANGLES and PT_FLAG_MOLLER_TRUMBORE apply as in a render; PT_FLAG_NO_AA and
 * PT_FLAG_REF_DISPATCH mean nothing here.  NaN or zero components get no special case and fall out of the IEEE
 * arithmetic, as for a query.
 *
 * Frames frame_first .. frame_first + n_frames - 1 of a ray are folded into rgba[i] in frame order by the render's
 * running mean: the first frame overwrites when accumulate_first = 0 (rgba is then never read) and averages over the
 * caller's values when it is 1; every later frame averages.  This is pt_render's rule.
 *
 * Consequence: with rays from pt_pixel_rays and seeds from pt_pixel_seeds, pt_trace(.., F, N, A, rgba) writes the
 * pixels of pt_render(F, N, A) on a PT_FLAG_NO_AA, one-ray-per-pixel context with that camera, bit for bit.
 *
 * Like a query, a trace is invisible to rendering: no timing events, launch counters, sweep or pool flags, tile
 * order, moments, presented state or captured graph, and nothing written that a render reads.
 *
 * n rays from host arrays, synchronous; rgba holds n * 4 floats, in and out.  seeds = NULL: seeds[i] =
 * (uint32)i * 923766u, the seeds of pixels (i, 0).  PT_E_STATE before pt_upload_scene; PT_E_ARG for a null rays or
 * rgba with n > 0, n < 0, frame_first < 1, n_frames < 1, frame_first + n_frames overflowing int, or accumulate_first
 * not 0 or 1; n = 0 is PT_OK without a launch.  A row-split context answers like any other. */
int pt_trace(pt_ctx* ctx, const pt_ray* rays, const unsigned* seeds, long long n, int frame_first, int n_frames,
             int accumulate_first, float* rgba);
/* The same on device arrays (d_rays and d_rgba 16-byte aligned, d_seeds 4-byte aligned or NULL; else PT_E_ARG),
 * enqueued on the context's stream (pt_stream) and not synchronised.  It allocates nothing. */
int pt_trace_device(pt_ctx* ctx, const void* d_rays, const void* d_seeds, long long n, int frame_first, int n_frames,
                    int accumulate_first, void* d_rgba);
/* The pixel part of the reference's seed, y * 831266u + x * 923766u, of n pixels xy = {x0, y0, ...}.  Pure host code. */
int pt_pixel_seeds(const int* xy, long long n, unsigned* seeds_out);
/* The trace on the host, of a scene in pt_upload_scene's arrays: packs it as pt_upload_scene does and runs the
 * device kernel's own per-ray code.  No device is touched.  ctx_flags, max_bounce, display_mode: what a context
 * would hold.  Returns the packer's error for a rejected scene. */
int pt_trace_host(const float* tris, int n_tris, const float* bvh, int n_nodes, const float* mats, int n_mats,
                  const float* spheres, int n_spheres, int ctx_flags, int max_bounce, int display_mode,
                  const pt_ray* rays, const unsigned* seeds, long long n, int frame_first, int n_frames,
                  int accumulate_first, float* rgba);

/* Camera models: depth of field, orthographic views and anti-aliased panoramas.  The camera is a
 * function of (pixel, frame, random state) evaluated inside the trace kernel: a lane makes its own ray at the start of
 * every path, so nothing is uploaded per sample and every frame of a call has its own jitter and lens sample.
 *
 * For pixel (x, y) of frame f the state starts as the reference's seed, y * 831266u + x * 923766u + f * 719393u, and
 * the camera takes its draws from it before Trace does, in this order: unless PT_CAM_NO_AA is set, ax then ay (the
 * reference's jitter; otherwise both are 0 and nothing is drawn); then the model's own, u1 then u2 for the thin lens
 * and none for the others.  u = (x + ax) / width - 0.5 and v = (y + ay) / height - 0.5.  With {pos, fwd, right, up}
 * as pt_set_camera derives them from cam (up scaled by height / width), upU = normalize(cross(right, fwd)) and
 * pi = 3.1415926f:
 *   PT_CAM_PINHOLE    o = pos, d = normalize(fwd + right u + up v): the built-in camera.
 *   PT_CAM_THIN_LENS  D = fwd + right u + up v, P = pos + D focus (the plane at distance `focus` along fwd is sharp),
 *                     r = aperture sqrt(u1), phi = 2 pi u2, o = pos + right r cos phi + upU r sin phi,
 *                     d = normalize(P - o).
 *   PT_CAM_ORTHO      o = pos + right (u ortho_width) + up (v ortho_width), d = fwd.
 *   PT_CAM_EQUIRECT   theta = 2 pi (u + 0.5), alpha = pi (v + 0.5), F = normalize(fwd.x, fwd.y, 0),
 *                     d = normalize((F (-cos theta) + right (-sin theta)) sin alpha + (0, 0, -cos alpha)), o = pos:
 *                     the centre column looks along F, columns to its right look to the right, row 0 looks down.
 * d is normalised and t_max = +inf.  The arithmetic is pinned (csrc/pt_camera.h) and the same on host and device.
 * Nothing is special-cased: a fwd parallel to z makes NaN rays, as it does in the reference.
 *
 * Frame f of pixel i = y * width + x is the reference's Trace from that ray and the state the camera left; the
 * frames of a pixel are folded into rgba[i] as pt_trace folds a ray's (pt_render's rule).  One ray per pixel: more
 * samples are more frames.
 *
 * Consequence: pt_trace_camera(PT_CAM_PINHOLE, flags 0, .., F, N, A, rgba) writes the pixels of pt_render(F, N, A) on
 * a default (flags 0, one-ray-per-pixel) context of that size and camera, bit for bit; with PT_CAM_NO_AA those of a
 * PT_FLAG_NO_AA context.
 *
 * The context's scene, max_bounce, display mode, PT_FLAG_NO_SKY, PT_FLAG_NO_SPHERES, PT_FLAG_NO_TRIANGLES and
 * PT_FLAG_MOLLER_TRUMBORE apply as in pt_trace; its PT_FLAG_NO_AA, PT_FLAG_REF_DISPATCH, size, camera and row split
 * mean nothing here: the camera's size and flag are its own.  Like a query and a trace, these calls are invisible to
 * rendering. */
#define PT_CAM_PINHOLE 0
#define PT_CAM_THIN_LENS 1
#define PT_CAM_ORTHO 2
#define PT_CAM_EQUIRECT 3
#define PT_CAM_NO_AA 1
typedef struct {
    int model;               /* PT_CAM_* */
    int width, height;       /* 1..65536, as pt_create allows */
    int flags;               /* PT_CAM_NO_AA */
    float cam[12];           /* as pt_set_camera */
    float aperture;          /* lens radius, thin lens; >= 0 */
    float focus;             /* distance of the plane in focus along fwd, thin lens; > 0 */
    float ortho_width;       /* world width of the view, ortho; > 0 */
    float pad;               /* 0 */
} pt_camera;                 /* 80 B */
/* Frames frame_first .. frame_first + n_frames - 1 of every pixel; rgba: a host array of width * height * 4 floats,
 * in and out, in the pixel order of pt_read_rgba32f on an unsplit context (row 0 = bottom).  Synchronous.
 * PT_E_STATE before pt_upload_scene; PT_E_ARG for the frame and accumulate_first errors of pt_trace, a null rgba or
 * camera, an unknown model or camera flag, a size out of range, and a NaN, negative or (focus, ortho_width) zero
 * aperture, focus or ortho_width for the model that reads it.  Fields a model does not read are ignored. */
int pt_trace_camera(pt_ctx* ctx, const pt_camera* camera, int frame_first, int n_frames, int accumulate_first,
                    float* rgba);
/* The same on a device array (16-byte aligned, else PT_E_ARG), enqueued on the context's stream (pt_stream) and not
 * synchronised.  It allocates nothing. */
int pt_trace_camera_device(pt_ctx* ctx, const pt_camera* camera, int frame_first, int n_frames, int accumulate_first,
                           void* d_rgba);
/* The same on the host, of a scene in pt_upload_scene's arrays: packs it as pt_upload_scene does and runs the device
 * kernel's own per-pixel code.  No device is touched.  Returns the packer's error for a rejected scene. */
int pt_trace_camera_host(const float* tris, int n_tris, const float* bvh, int n_nodes, const float* mats, int n_mats,
                         const float* spheres, int n_spheres, int ctx_flags, int max_bounce, int display_mode,
                         const pt_camera* camera, int frame_first, int n_frames, int accumulate_first, float* rgba);
/* The ray of each of the n pixels xy = {x0, y0, ...} in frame `frame` (>= 1), and in states_out (may be NULL) the
 * random state after the camera's draws: pt_trace of rays_out[i] with seed states_out[i] - frame * 719393u is that
 * pixel's frame.  Pure host code.  PT_E_ARG also for a pixel outside the image (nothing is written then). */
int pt_camera_rays_host(const pt_camera* camera, const int* xy, long long n, int frame, pt_ray* rays_out,
                        unsigned* states_out);
/* The same for every pixel of the image, in pixel order, into device arrays (d_rays 16-byte aligned, width * height
 * rays; d_states 4-byte aligned or NULL), enqueued on the context's stream and not synchronised: the input of a
 * pt_intersect_device (a depth buffer through the lens) or a pt_trace_device.  Needs no uploaded scene. */
int pt_camera_rays_device(pt_ctx* ctx, const pt_camera* camera, int frame, void* d_rays, void* d_states);

/* Film: the running image, the luminance moments and the first-hit guides of one pt_camera on one
 * context, kept on the device and written in one pass over the paths -- what a camera-model render needs to be
 * rendered to a noise level (pt_film_noise, pt_film_expose_until) and shown denoised meanwhile (pt_film_denoise).
 *
 * For a film of camera cam, width x height pixels, guide_frames = G >= 1, every plane bit for bit:
 *   image    after pt_film_expose(F, N, A) what pt_trace_camera_device(cam, F, N, A, image) writes.
 *   moments  (S1, S2) per pixel as in "Per-pixel noise estimate" above: for each frame of the call, in frame order,
 *            Y of that frame's path colour (the colour that enters the running mean, not the mean), S1 += Y,
 *            S2 += Y*Y.  An exposure with accumulate_first = 0 starts from (0, 0) and sets the film's frame count
 *            n = N; with 1 it continues and n += N.
 *   guides   two quads per pixel, (N.rgb, Z) and (A.rgb, 0).  N, A and Z are the rgb, rgb and .x of
 *            pt_trace_camera(cam, 1, G, 0) on a context whose display mode is 2, 3 and 4 (same scene, flags and
 *            max_bounce): functions of a path's first segment, which the exposure that passes through a frame
 *            f <= G takes from the first hit it casts anyway.  The context's own display mode governs the radiance
 *            only, never the guides.  The film keeps guides_held, the largest h such that frames 1..h are folded in
 *            (h <= G): an exposure whose range contains frame h + 1 raises h to min(G, its last frame); any other
 *            leaves the guides alone.  They do not depend on accumulate_first and are reset (h = 0) only by
 *            pt_film_set_camera, by another guide_frames, or when the context's scene has been replaced.
 * One ray per pixel; a row-split context answers for the whole width x height, like a trace.
 *
 * A film is invisible to rendering, as a query and a trace are: no timing events, launch counters, tile order,
 * context moments or captured graph.  Everything is enqueued on the context's stream (pt_stream); only create and
 * destroy allocate.  Errors follow pt_trace_camera's: PT_E_STATE before pt_upload_scene; PT_E_ARG for frame ranges,
 * flags and null pointers. */
typedef struct pt_film pt_film;
/* width * height must be below 2^31.  The film starts black, n = 0, guides_held = 0.  Needs no uploaded scene. */
int pt_film_create(pt_ctx* ctx, const pt_camera* camera, int guide_frames, pt_film** out);
/* Waits for the context's stream.  Before pt_destroy of its context. */
void pt_film_destroy(pt_film* film);
/* Another camera of the same width x height (else PT_E_ARG); guides_held = 0.  The image and the moments stay the
 * caller's business, as on a context: the next exposure with accumulate_first = 0 restarts them. */
int pt_film_set_camera(pt_film* film, const pt_camera* camera);
/* Frames frame_first .. frame_first + n_frames - 1 of every pixel.  Enqueued, not waited for. */
int pt_film_expose(pt_film* film, int frame_first, int n_frames, int accumulate_first);
/* The summary of every pixel, q = quantise(S1, S2, n), pixels = width * height, reduced on the device (integers
 * only: exact in any order).  Waits.  PT_E_STATE: n < 2. */
int pt_film_noise(pt_film* film, float target, pt_noise_stats* out);
/* pt_render_until's rule on a film: exposes `batch` frames at a time (the first batch with the caller's
 * accumulate_first, the rest accumulating; the last batch may be shorter) and stops after the first batch with
 * sum_q <= (unsigned)(target * 65536.0f) * pixels, or after max_frames.  The image afterwards is that of
 * pt_film_expose(frame_first, *frames_done, accumulate_first), bit for bit.  `last` may be NULL.
 * PT_E_ARG: batch < 2, max_frames < batch or target <= 0. */
int pt_film_expose_until(pt_film* film, int frame_first, int accumulate_first, int batch, int max_frames,
                         float target, int* frames_done, pt_noise_stats* last);
/* pt_denoise's filter on the film's planes, the whole image its footprint: guided by the variance of the mean
 * luminance when n >= 2.  If guides_held < params->guide_frames the guides are completed first by a guides-only
 * launch of frames guides_held + 1 .. G, whose paths end after the first segment and which touches neither the image
 * nor the moments; a guide_frames other than the film's becomes the film's and re-gathers them.  Enqueued, not waited
 * for.  params NULL = pt_denoise_defaults (guide_frames 4); info may be NULL (guides_rendered: that launch ran). */
int pt_film_denoise(pt_film* film, const pt_denoise_params* params, pt_denoise_info* info);
/* n and guides_held (0 after the context's scene was replaced).  Either pointer may be NULL. */
int pt_film_info(pt_film* film, int* frames, int* guides_held);
#define PT_FILM_IMAGE 0          /* W*H*4 float */
#define PT_FILM_MOMENTS 1        /* W*H*2 float */
#define PT_FILM_GUIDES 2         /* W*H*8 float, pt_read_guides' order */
#define PT_FILM_DENOISED 3       /* W*H*4 float; PT_E_STATE before a denoise */
#define PT_FILM_IMAGE_ACES8 4    /* W*H*4 bytes, the ACES view computed on the device */
#define PT_FILM_DENOISED_ACES8 5
/* Waits for the context's stream, then copies the plane.  PT_E_ARG: bytes is not the plane's size. */
int pt_film_read(pt_film* film, int what, void* host_dst, size_t bytes);
/* The device planes 0..3, for a client's own kernels on the context's stream.  On the device the guides are two
 * planes, not interleaved: (N.rgb, Z) of every pixel, then (A.rgb, 0) of every pixel. */
int pt_film_device(pt_film* film, int what, void** dev_ptr, size_t* bytes);
/* An exposure on the host, of a scene in pt_upload_scene's arrays: packs it as pt_upload_scene does and runs the
 * device kernel's own per-pixel code.  No device is touched.  rgba (W*H*4), moments (W*H*2) and guides (W*H*8, as
 * PT_FILM_GUIDES) are in and out; frames_before (>= 0) and guides_held (0..guide_frames) are the film's n and h before
 * the call, *guides_held_out (may be NULL) is h after it.  Returns the packer's error for a rejected scene. */
int pt_film_expose_host(const float* tris, int n_tris, const float* bvh, int n_nodes, const float* mats, int n_mats,
                        const float* spheres, int n_spheres, int ctx_flags, int max_bounce, int display_mode,
                        const pt_camera* camera, int guide_frames, int frame_first, int n_frames, int accumulate_first,
                        int frames_before, int guides_held, float* rgba, float* moments, float* guides,
                        int* guides_held_out);

#ifdef __cplusplus
}
#endif
#endif /* PT_API_H */
