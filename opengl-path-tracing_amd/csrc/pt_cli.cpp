// ptrace -- headless C++ host driver: the reference's main.cpp/run() without the window.
//
//   main.cpp:6-11, ogl_path_trace.h:71-216 (run), :367-530 (setupBuffers)
// The reference ignores argv and hard-codes scene_data/freeobj.txt (absent from the repo,
// SURVEY.md §0.1); this driver honours the README's intent (readme.md:8-9): the .obj and
// .mtl come from the command line.  Frames f = 1..spp are rendered with accumulate = 0
// on frame 1 (ogl_path_trace.h:160-204 after a reset), fused `chunk` frames per launch,
// optionally row-split across several GPUs of this node: --ranks R contexts (rank r on device
// r mod G), the scene validated once and broadcast, the frame gathered over RCCL (pt_group.h).
//
// Output: RGBA32F accumulation as PFM (row 0 = bottom, like the GL texture) and the
// ACES-tonemapped RGBA8 view as binary PPM (screenQuadFrag.c).
#include "../../include/pt_api.h"
#include "../../include/pt_group.h"
#include "../../include/pt_scene.h"
#include "../../include/pt_viewer.h"

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

static void usage() {
    std::fprintf(stderr,
                 "usage: ptrace <scene.obj> <scene.mtl | -> [--width W] [--height H] [--spp S] [--chunk C]\n"
                 "              [--bounces B] [--mode 1..4] [--gpus G] [--ranks R] [--pfm out.pfm] [--ppm out.ppm]\n"
                 "              [--camera px py pz dx dy dz] [--robust] [--events script.txt]\n"
                 "  --robust  general Wavefront ingest (v/vt/vn corners, polygons, negative indices,\n"
                 "            free-form MTL; '-' as the MTL uses the OBJ's mtllib)\n"
                 "  --events  replay a recorded interactive session instead of --spp frames: the\n"
                 "            reference's render loop with its camera controller and accumulation\n"
                 "            reset (include/pt_viewer.h).  Script lines:\n"
                 "              frame T            one loop iteration at glfwGetTime() = T seconds\n"
                 "              frames N T0 DT     N iterations at T0, T0+DT, ...\n"
                 "              key K ACTION       key callback; K = GLFW code or w a s d 1-4 space shift esc,\n"
                 "                                 ACTION = press | release | repeat\n"
                 "              cursor X Y         cursor callback\n"
                 "            '#' starts a comment; the loop ends early once esc was pressed\n"
                 "  --gpus G        devices 0..G-1 of this node\n"
                 "  --ranks R       row-split contexts (default G; rank r renders rows r, r+R, ... on device\n"
                 "                  r mod G); the frame is gathered over RCCL on device 0\n"
                 "  --checkpoint F  after rendering, save the RGBA32F accumulation and the next frame\n"
                 "                  number (text header 'PTCK2 W H next_frame bounces mode tris nodes' + the\n"
                 "                  camera's 6 floats, then W*H*4 floats)\n"
                 "  --resume F      continue a saved accumulation: frames next_frame.. with accumulate = 1,\n"
                 "                  the same image as one uninterrupted run\n"
                 "  --noise-target X  render until the mean per-pixel relative error (standard error of the\n"
                 "                  mean luminance over the mean, pt_api.h: pt_render_until) is at most X,\n"
                 "                  checked every --batch B frames (default 16), at most --max-spp N frames\n"
                 "                  (default --spp); one GPU, not with --resume or --events\n"
                 "  --adaptive      with --noise-target: every work-queue tile stops on its own once its mean\n"
                 "                  relative error meets the target (pt_api.h: pt_render_adaptive)\n"
                 "  --spp-map F     with --adaptive: the frames each tile received as a binary PGM, one pixel\n"
                 "                  per tile, top row first (16-bit when a count exceeds 255)\n"
                 "  --json          print a JSON summary line (with --noise-target also frames_done,\n"
                 "                  noise_mean, noise_max, noise_above_frac; with --adaptive also tiles,\n"
                 "                  tiles_active, pixel_frames)\n"
                 "  --gpu-bvh       build the BVH on GPU 0 (pt_bvh_build_gpu; the same nodes)\n"
                 "  --denoise       after rendering, filter the image (pt_api.h: pt_denoise; one context) with\n"
                 "                  --denoise-iters N iterations (default 5) over guides of --guide-frames G\n"
                 "                  frames (default 4); --denoise-pfm F / --denoise-ppm F write the result as\n"
                 "                  the RGBA32F PFM / the ACES PPM; --json gains a \"denoise\" object\n"
                 "  --pick X,Y      what is under pixel (X, Y), row 0 = bottom (pt_api.h: pt_pick; repeatable): one\n"
                 "                  JSON line per pixel with kind (0 miss, 1 sphere, 2 triangle), prim, mat, t, n,\n"
                 "                  p and the material's albedo (t and albedo null for a miss)\n"
                 "  --rays F --hits G [--any-hit]  cast the raw 32-byte rays of F (pt_api.h: pt_ray, pt_intersect)\n"
                 "                  and write the raw 48-byte hit records to G\n"
                 "  --rays F --radiance G [--seeds S] [--spp N]  trace the rays of F (pt_api.h: pt_trace), frames 1..N\n"
                 "                  (default 1), and write one raw RGBA32F record per ray to G; S: one raw uint32 seed\n"
                 "                  per ray (default: those of pixels (i, 0)); with --spp, --pick lines gain\n"
                 "                  \"radiance\", the traced colour of the pixel's ray over frames 1..N\n"
                 "                  queries run on context 0 after the render; without --spp, --noise-target and\n"
                 "                  --events they run alone: nothing is rendered and no image is written\n"
                 "  --camera-model pinhole|thinlens|ortho|equirect  render frames 1..--spp through a camera model\n"
                 "                  (pt_api.h: pt_camera, pt_trace_camera), --chunk frames per call, at --width x\n"
                 "                  --height from --camera; the image is stored in the context, so --pfm, --ppm, --json\n"
                 "                  and --pick work as ever.  --aperture R (lens radius) and --focus D (distance of the\n"
                 "                  sharp plane along the view direction) or --focus-at X,Y (D = dot(p - pos, fwd) of\n"
                 "                  what --pick finds under that pixel, in binary32) for thinlens; --ortho-width W (world\n"
                 "                  width of the view) for ortho; --no-aa: no jitter.  One context only: not with --gpus\n"
                 "                  above 1, --ranks, --adaptive, --noise-target, --denoise*, --events, --checkpoint,\n"
                 "                  --resume, --rays, --hits, --radiance or --seeds\n"
                 "  --film          with --camera-model: the frames go through a film (pt_api.h: pt_film), which keeps\n"
                 "                  moments and first-hit guides of that camera beside the image, so that --noise-target X\n"
                 "                  [--batch B] [--max-spp N] (pt_film_expose_until) and --denoise [--denoise-iters N]\n"
                 "                  [--guide-frames G] [--denoise-pfm F] [--denoise-ppm F] (pt_film_denoise) work, and\n"
                 "                  --pfm, --ppm and --json are of the film's planes; --json gains a \"film\" object\n");
}

// Checkpoint of a progressive render (SURVEY.md §5 checkpoint / resume): the running mean
// (computeShader.c:548-551) only needs the accumulation image and the next frame number.
// The header also records what the running mean depends on besides the image -- bounces,
// display mode, the scene's triangle and node counts and the camera -- and --resume refuses a
// checkpoint that does not match them (a silent blend of two different renders otherwise).
struct CkptKey {
    int bounces, mode, tris, nodes;
    float cam[6];
};

static bool save_checkpoint(const std::string& path, int W, int H, int next_frame, const CkptKey& key,
                            const std::vector<float>& img) {
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    std::fprintf(f, "PTCK2 %d %d %d %d %d %d %d %.9g %.9g %.9g %.9g %.9g %.9g\n", W, H, next_frame, key.bounces,
                 key.mode, key.tris, key.nodes, key.cam[0], key.cam[1], key.cam[2], key.cam[3], key.cam[4], key.cam[5]);
    const bool ok = std::fwrite(img.data(), 4, img.size(), f) == img.size();
    return std::fclose(f) == 0 && ok;
}

static bool load_checkpoint(const std::string& path, int W, int H, int& next_frame, CkptKey& key,
                            std::vector<float>& img, std::string& err) {
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) { err = "cannot open " + path; return false; }
    int w = 0, h = 0, nf = 0;
    char magic[8] = {0};
    bool ok = std::fscanf(f, "%5s %d %d %d %d %d %d %d %g %g %g %g %g %g", magic, &w, &h, &nf, &key.bounces, &key.mode,
                          &key.tris, &key.nodes, &key.cam[0], &key.cam[1], &key.cam[2], &key.cam[3], &key.cam[4],
                          &key.cam[5]) == 14 &&
              std::string(magic) == "PTCK2" && std::fgetc(f) == '\n';
    if (!ok) err = path + ": not a PTCK2 checkpoint";
    else if (w != W || h != H) { ok = false; err = path + ": checkpoint is " + std::to_string(w) + "x" + std::to_string(h); }
    else if (nf < 1) { ok = false; err = path + ": bad next frame"; }
    if (ok) {
        img.assign(4 * (size_t)W * H, 0.0f);
        ok = std::fread(img.data(), 4, img.size(), f) == img.size();
        if (!ok) err = path + ": truncated";
        next_frame = nf;
    }
    std::fclose(f);
    return ok;
}

// One event of an --events script (see usage()).
struct Event {
    int kind;          // 0 frame, 1 key, 2 cursor
    double a, b;
    int key, action;
};

static bool parse_events(const char* path, std::vector<Event>& ev, std::string& err) {
    std::ifstream in(path);
    if (!in) { err = std::string("cannot open ") + path; return false; }
    std::string line;
    int ln = 0;
    while (std::getline(in, line)) {
        ln++;
        const size_t hash = line.find('#');
        if (hash != std::string::npos) line.resize(hash);
        std::istringstream ss(line);
        std::string op;
        if (!(ss >> op)) continue;
        Event e = {0, 0.0, 0.0, 0, 0};
        bool ok = true;
        if (op == "frame") {
            ok = static_cast<bool>(ss >> e.a);
            ev.push_back(e);
        } else if (op == "frames") {
            long n = 0;
            double t0 = 0, dt = 0;
            ok = static_cast<bool>(ss >> n >> t0 >> dt) && n >= 0 && n <= 10000000;
            for (long i = 0; ok && i < n; i++) { e.a = t0 + (double)i * dt; ev.push_back(e); }
        } else if (op == "key") {
            std::string k, a;
            ok = static_cast<bool>(ss >> k >> a);
            e.kind = 1;
            if (k == "w" || k == "W") e.key = PT_KEY_W;
            else if (k == "a" || k == "A") e.key = PT_KEY_A;
            else if (k == "s" || k == "S") e.key = PT_KEY_S;
            else if (k == "d" || k == "D") e.key = PT_KEY_D;
            else if (k == "space") e.key = PT_KEY_SPACE;
            else if (k == "shift") e.key = PT_KEY_LEFT_SHIFT;
            else if (k == "esc") e.key = PT_KEY_ESCAPE;
            else if (k.size() == 1 && k[0] >= '1' && k[0] <= '4') e.key = PT_KEY_1 + (k[0] - '1');
            else e.key = std::atoi(k.c_str());
            if (a == "press") e.action = PT_PRESS;
            else if (a == "release") e.action = PT_RELEASE;
            else if (a == "repeat") e.action = PT_REPEAT;
            else e.action = std::atoi(a.c_str());
            ev.push_back(e);
        } else if (op == "cursor") {
            e.kind = 2;
            ok = static_cast<bool>(ss >> e.a >> e.b);
            ev.push_back(e);
        } else {
            ok = false;
        }
        if (!ok) { err = std::string(path) + ":" + std::to_string(ln) + ": bad event line"; return false; }
    }
    return true;
}

#define CHECK(expr, ctx)                                                              \
    do {                                                                              \
        int rc_ = (expr);                                                             \
        if (rc_) {                                                                    \
            std::fprintf(stderr, "%s failed (%d): %s\n", #expr, rc_, pt_last_error(ctx)); \
            return 1;                                                                 \
        }                                                                             \
    } while (0)

int main(int argc, char** argv) {
    if (argc < 3) { usage(); return 2; }
    const char* obj = argv[1];
    const char* mtl = argv[2];
    int W = 1000, H = 800, spp = 64, chunk = 16, bounces = 5, mode = 1, gpus = 1, ranks = 0;   // ogl_path_trace.h:45-46
    std::string pfm = "out.pfm", ppm = "out.ppm";
    float cam[12] = {0, -6, 1, 0, 0, 1, 0, 0, 0, 0, 0, 0};                          // ogl_path_trace.h:53-54
    bool robust = false, json = false, gpu_bvh = false;
    const char* events = nullptr;
    std::string checkpoint, resume;
    float noise_target = 0.0f;            // > 0: render until converged (pt_render_until)
    int batch = 16, max_spp = 0;
    bool until = false, adaptive = false;
    std::string spp_map;
    pt_adaptive_stats astats = {{0, 0, 0, 0, 0}, 0, 0, 0};
    bool denoise = false;
    pt_denoise_params dparams;
    pt_denoise_defaults(&dparams);
    pt_denoise_info dinfo = {0, 0, 0, 0};
    std::string denoise_pfm, denoise_ppm;
    double denoise_ms = 0.0;
    std::vector<int> picks;               // x, y pairs
    std::string rays_path, hits_path, radiance_path, seeds_path;
    bool any_hit = false, spp_given = false;
    int cam_model = -1;                   // >= 0: render through pt_trace_camera
    pt_camera pcam = {PT_CAM_PINHOLE, 0, 0, 0, {0}, 0.0f, 1.0f, 1.0f, 0.0f};
    bool focus_at = false, lens_given = false, ranks_given = false;
    bool use_film = false;                // the camera model's frames go through a pt_film
    int film_frames = 0, film_held = 0;
    int focus_xy[2] = {0, 0};
    for (int i = 3; i < argc; i++) {
        std::string a = argv[i];
        auto next = [&](void) -> const char* { if (i + 1 >= argc) { usage(); std::exit(2); } return argv[++i]; };
        if (a == "--width") W = std::atoi(next());
        else if (a == "--height") H = std::atoi(next());
        else if (a == "--spp") { spp = std::atoi(next()); spp_given = true; }
        else if (a == "--chunk") chunk = std::atoi(next());
        else if (a == "--bounces") bounces = std::atoi(next());
        else if (a == "--mode") mode = std::atoi(next());
        else if (a == "--gpus") gpus = std::atoi(next());
        else if (a == "--ranks") { ranks = std::atoi(next()); ranks_given = true; }
        else if (a == "--pfm") pfm = next();
        else if (a == "--ppm") ppm = next();
        else if (a == "--camera") { for (int k = 0; k < 6; k++) cam[k < 3 ? k : k + 1] = (float)std::atof(next()); }
        else if (a == "--robust") robust = true;
        else if (a == "--events") events = next();
        else if (a == "--checkpoint") checkpoint = next();
        else if (a == "--resume") resume = next();
        else if (a == "--noise-target") { noise_target = (float)std::atof(next()); until = true; }
        else if (a == "--adaptive") adaptive = true;
        else if (a == "--spp-map") spp_map = next();
        else if (a == "--batch") batch = std::atoi(next());
        else if (a == "--max-spp") max_spp = std::atoi(next());
        else if (a == "--json") json = true;
        else if (a == "--gpu-bvh") gpu_bvh = true;
        else if (a == "--denoise") denoise = true;
        else if (a == "--denoise-iters") dparams.iterations = std::atoi(next());
        else if (a == "--guide-frames") dparams.guide_frames = std::atoi(next());
        else if (a == "--denoise-pfm") denoise_pfm = next();
        else if (a == "--denoise-ppm") denoise_ppm = next();
        else if (a == "--pick") {
            int x = 0, y = 0;
            if (std::sscanf(next(), "%d,%d", &x, &y) != 2) { usage(); return 2; }
            picks.push_back(x);
            picks.push_back(y);
        }
        else if (a == "--rays") rays_path = next();
        else if (a == "--hits") hits_path = next();
        else if (a == "--any-hit") any_hit = true;
        else if (a == "--radiance") radiance_path = next();
        else if (a == "--seeds") seeds_path = next();
        else if (a == "--camera-model") {
            const std::string m = next();
            cam_model = m == "pinhole" ? PT_CAM_PINHOLE : m == "thinlens" ? PT_CAM_THIN_LENS : m == "ortho" ? PT_CAM_ORTHO
                      : m == "equirect" ? PT_CAM_EQUIRECT : -1;
            if (cam_model < 0) { std::fprintf(stderr, "--camera-model is one of pinhole, thinlens, ortho, equirect\n"); return 2; }
        }
        else if (a == "--aperture") { pcam.aperture = (float)std::atof(next()); lens_given = true; }
        else if (a == "--focus") { pcam.focus = (float)std::atof(next()); lens_given = true; }
        else if (a == "--focus-at") {
            if (std::sscanf(next(), "%d,%d", &focus_xy[0], &focus_xy[1]) != 2) { usage(); return 2; }
            focus_at = lens_given = true;
        }
        else if (a == "--ortho-width") { pcam.ortho_width = (float)std::atof(next()); lens_given = true; }
        else if (a == "--no-aa") { pcam.flags |= PT_CAM_NO_AA; lens_given = true; }
        else if (a == "--film") use_film = true;
        else { usage(); return 2; }
    }
    if (ranks == 0) ranks = gpus;
    if (use_film && cam_model < 0) {
        std::fprintf(stderr, "--film needs --camera-model\n");
        return 2;
    }
    if (cam_model < 0 && lens_given) {
        std::fprintf(stderr, "--aperture, --focus, --focus-at, --ortho-width and --no-aa need --camera-model\n");
        return 2;
    }
    if (cam_model >= 0) {
        // one context, frames 1..spp, nothing that owns the render loop or the traced-ray options
        // (a film brings the moments and the guides of the camera model: --noise-target and --denoise work on it)
        const char* clash = gpus > 1 ? "--gpus above 1" : ranks_given ? "--ranks" : adaptive ? "--adaptive"
                          : (until && !use_film) ? "--noise-target"
                          : ((denoise || !denoise_pfm.empty() || !denoise_ppm.empty()) && !use_film) ? "--denoise"
                          : events ? "--events" : !checkpoint.empty() ? "--checkpoint" : !resume.empty() ? "--resume"
                          : !rays_path.empty() ? "--rays" : !hits_path.empty() ? "--hits" : !radiance_path.empty() ? "--radiance"
                          : !seeds_path.empty() ? "--seeds" : nullptr;
        if (clash) { std::fprintf(stderr, "--camera-model excludes %s\n", clash); return 2; }
    }
    if (spp < 1 || chunk < 1 || gpus < 1 || ranks < 1) { usage(); return 2; }
    if (events && (!resume.empty() || !checkpoint.empty())) {
        std::fprintf(stderr, "--events excludes --resume / --checkpoint\n");
        return 2;
    }
    if (denoise && (gpus > 1 || ranks > 1)) {     // a row-split context has no neighbouring rows to filter over
        std::fprintf(stderr, "--denoise excludes --gpus / --ranks above 1\n");
        return 2;
    }
    if (!denoise && (!denoise_pfm.empty() || !denoise_ppm.empty())) {
        std::fprintf(stderr, "--denoise-pfm / --denoise-ppm need --denoise\n");
        return 2;
    }
    if (rays_path.empty() != (hits_path.empty() && radiance_path.empty()) || (any_hit && hits_path.empty()) ||
        (!seeds_path.empty() && radiance_path.empty())) {
        std::fprintf(stderr, "--rays goes with --hits or --radiance, --any-hit with --hits, --seeds with --radiance\n");
        return 2;
    }
    const int trace_frames = spp_given ? spp : 1;   // of --radiance and of a --pick line's colour
    const bool queries = !picks.empty() || !rays_path.empty();
    const bool query_only = queries && !spp_given && !until && !events && !denoise && resume.empty() && checkpoint.empty() &&
                            cam_model < 0;
    if (adaptive && !until) {
        std::fprintf(stderr, "--adaptive needs --noise-target\n");
        return 2;
    }
    if (!spp_map.empty() && !adaptive) {
        std::fprintf(stderr, "--spp-map needs --adaptive\n");
        return 2;
    }
    if (until) {
        // one context only: pt_render_until is not defined across a group, the moments are not
        // part of a checkpoint, and an event script resets the image on its own schedule
        if (gpus > 1 || ranks > 1 || !resume.empty() || events) {
            std::fprintf(stderr, "--noise-target excludes --gpus / --ranks above 1, --resume and --events\n");
            return 2;
        }
        if (max_spp == 0) max_spp = spp;
        if (!(noise_target > 0.0f) || batch < 2 || max_spp < batch) {
            std::fprintf(stderr, "--noise-target needs a target > 0, --batch >= 2 and --max-spp >= --batch\n");
            return 2;
        }
    }
    int first = 1;                        // frame number of the first frame rendered
    std::vector<float> prior;
    CkptKey saved = {};
    if (!resume.empty()) {
        std::string err;
        if (!load_checkpoint(resume, W, H, first, saved, prior, err)) { std::fprintf(stderr, "%s\n", err.c_str()); return 2; }
    }

    auto t0 = std::chrono::steady_clock::now();
    pt_scene* sc = nullptr;
    const bool mtl_from_obj = std::string(mtl) == "-";
    if (mtl_from_obj && !robust) { std::fprintf(stderr, "'-' as the MTL needs --robust\n"); return 2; }
    int rc = pt_scene_load_obj_ex(obj, mtl_from_obj ? nullptr : mtl, robust ? PT_LOAD_ROBUST : PT_LOAD_REFERENCE, &sc);
    if (!rc) rc = pt_scene_add_builtins(sc);
    if (!rc) rc = gpu_bvh ? pt_scene_build_bvh_gpu(sc, 0) : pt_scene_build_bvh(sc);
    if (rc) { std::fprintf(stderr, "scene: %s (%d)\n", pt_scene_last_error(sc), rc); pt_scene_free(sc); return 1; }
    int cnt[5];
    pt_scene_counts(sc, cnt);
    std::vector<float> tris(16 * (size_t)cnt[0]), mats(16 * (size_t)cnt[1]), sph(8 * (size_t)cnt[2]), nodes(12 * (size_t)cnt[3]);
    pt_scene_get_tris(sc, tris.data(), cnt[0]);
    pt_scene_get_mats(sc, mats.data(), cnt[1]);
    pt_scene_get_spheres(sc, sph.data(), cnt[2]);
    pt_scene_get_nodes(sc, nodes.data(), cnt[3]);
    pt_scene_free(sc);
    double t_scene = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::printf("# of polygons: %d  # of materials: %d (+5 built-in)  # of spheres: %d  BVH nodes: %d  (%.3f s)\n",
                cnt[0], cnt[4], cnt[2], cnt[3], t_scene);
    const CkptKey key = {bounces, mode, cnt[0], cnt[3], {cam[0], cam[1], cam[2], cam[4], cam[5], cam[6]}};
    if (!resume.empty() &&
        (saved.bounces != key.bounces || saved.mode != key.mode || saved.tris != key.tris || saved.nodes != key.nodes ||
         std::memcmp(saved.cam, key.cam, sizeof(key.cam)) != 0)) {
        std::fprintf(stderr, "%s: checkpoint of a different render (bounces %d mode %d tris %d nodes %d camera "
                             "%g %g %g %g %g %g); refusing to blend\n", resume.c_str(), saved.bounces, saved.mode,
                     saved.tris, saved.nodes, saved.cam[0], saved.cam[1], saved.cam[2], saved.cam[3], saved.cam[4],
                     saved.cam[5]);
        return 2;
    }

    const int nctx = ranks;
    std::vector<pt_ctx*> ctx(nctx, nullptr);
    for (int g = 0; g < nctx; g++) {
        pt_config cfg = {W, H, bounces, mode, 0, 1, g % gpus, g, nctx};
        CHECK(pt_create(&cfg, &ctx[g]), ctx[g]);
    }
    pt_group* group = nullptr;
    if (nctx > 1) {   // one RCCL communicator over the devices; the scene is validated once
        int grc = pt_group_create(ctx.data(), nctx, &group);
        if (!grc) grc = pt_group_upload_scene(group, tris.data(), cnt[0], nodes.data(), cnt[3], mats.data(), cnt[1],
                                              sph.data(), cnt[2]);
        if (grc) { std::fprintf(stderr, "pt_group: %s (%d)\n", pt_group_last_error(group), grc); return 1; }
    }
    for (int g = 0; g < nctx; g++) {
        if (!group)
            CHECK(pt_upload_scene(ctx[g], tris.data(), cnt[0], nodes.data(), cnt[3], mats.data(), cnt[1], sph.data(), cnt[2]), ctx[g]);
        CHECK(pt_set_camera(ctx[g], cam), ctx[g]);
        if (!prior.empty()) {             // this context's rows of the saved image
            int rows = 0, r0 = 0, rs = 1;
            pt_rows(ctx[g], &rows, &r0, &rs);
            std::vector<float> part(4 * (size_t)rows * W);
            for (int k = 0; k < rows; k++)
                std::memcpy(&part[4 * (size_t)k * W], &prior[4 * (size_t)(r0 + k * rs) * W], 16 * (size_t)W);
            CHECK(pt_write_rgba32f(ctx[g], part.data(), part.size() * 4), ctx[g]);
        }
    }
    // the ray queries (--pick, --rays / --hits), on context 0: every context holds the whole scene
    auto run_queries = [&]() -> int {
        if (!picks.empty()) {
            std::vector<pt_hit> h(picks.size() / 2);
            CHECK(pt_pick(ctx[0], picks.data(), (long long)h.size(), h.data()), ctx[0]);
            std::vector<float> colour(4 * h.size());
            if (spp_given) {                  // the radiance behind the pixel: its ray and its seed, frames 1..spp
                std::vector<pt_ray> pr(h.size());
                std::vector<unsigned> ps(h.size());
                if (pt_pixel_rays(W, H, cam, picks.data(), (long long)h.size(), pr.data()) ||
                    pt_pixel_seeds(picks.data(), (long long)h.size(), ps.data())) return 1;
                CHECK(pt_trace(ctx[0], pr.data(), ps.data(), (long long)h.size(), 1, trace_frames, 0, colour.data()), ctx[0]);
            }
            for (size_t i = 0; i < h.size(); i++) {
                std::printf("{\"pick\": [%d, %d], \"kind\": %d, \"prim\": %d, \"mat\": %d, ", picks[2 * i], picks[2 * i + 1],
                            h[i].kind, h[i].prim, h[i].mat);
                if (h[i].kind == PT_HIT_NONE) std::printf("\"t\": null, ");
                else std::printf("\"t\": %.9g, ", h[i].t);
                std::printf("\"n\": [%.9g, %.9g, %.9g], \"p\": [%.9g, %.9g, %.9g], ", h[i].n[0], h[i].n[1], h[i].n[2],
                            h[i].p[0], h[i].p[1], h[i].p[2]);
                if (h[i].kind == PT_HIT_NONE) std::printf("\"albedo\": null");
                else std::printf("\"albedo\": [%.9g, %.9g, %.9g]", mats[16 * (size_t)h[i].mat], mats[16 * (size_t)h[i].mat + 1],
                                 mats[16 * (size_t)h[i].mat + 2]);
                if (spp_given) std::printf(", \"radiance\": [%.9g, %.9g, %.9g]", colour[4 * i], colour[4 * i + 1], colour[4 * i + 2]);
                std::printf("}\n");
            }
        }
        if (!rays_path.empty()) {
            FILE* f = std::fopen(rays_path.c_str(), "rb");
            if (!f) { std::fprintf(stderr, "cannot read %s\n", rays_path.c_str()); return 1; }
            std::vector<pt_ray> rays;
            pt_ray r;
            while (std::fread(&r, sizeof(r), 1, f) == 1) rays.push_back(r);
            std::fclose(f);
            if (!hits_path.empty()) {
                std::vector<pt_hit> h(rays.size());
                CHECK(pt_intersect(ctx[0], rays.data(), (long long)rays.size(), h.data(), any_hit ? PT_QUERY_ANY_HIT : 0), ctx[0]);
                f = std::fopen(hits_path.c_str(), "wb");
                if (!f || std::fwrite(h.data(), sizeof(pt_hit), h.size(), f) != h.size()) {
                    std::fprintf(stderr, "cannot write %s\n", hits_path.c_str());
                    return 1;
                }
                std::fclose(f);
            }
            if (!radiance_path.empty()) {
                std::vector<unsigned> seeds;
                if (!seeds_path.empty()) {
                    seeds.resize(rays.size());
                    f = std::fopen(seeds_path.c_str(), "rb");
                    const bool ok = f && std::fread(seeds.data(), sizeof(unsigned), seeds.size(), f) == seeds.size();
                    if (f) std::fclose(f);
                    if (!ok) { std::fprintf(stderr, "%s: cannot read one seed per ray\n", seeds_path.c_str()); return 1; }
                }
                std::vector<float> rgba(4 * rays.size());
                CHECK(pt_trace(ctx[0], rays.data(), seeds.empty() ? nullptr : seeds.data(), (long long)rays.size(), 1,
                               trace_frames, 0, rgba.data()), ctx[0]);
                f = std::fopen(radiance_path.c_str(), "wb");
                if (!f || std::fwrite(rgba.data(), 16, rays.size(), f) != rays.size()) {
                    std::fprintf(stderr, "cannot write %s\n", radiance_path.c_str());
                    return 1;
                }
                std::fclose(f);
            }
        }
        return 0;
    };
    if (query_only) {
        const int qrc = run_queries();
        pt_group_destroy(group);
        for (int g = 0; g < nctx; g++) pt_destroy(ctx[g]);
        return qrc;
    }
    auto t1 = std::chrono::steady_clock::now();
    int frames_run = 0, resets = 0;
    pt_noise_stats noise = {0, 0, 0, 0, 0};
    pt_film* film = nullptr;
    if (events) {
        // the reference's render loop (ogl_path_trace.h:160-204) driven by a recorded session
        std::vector<Event> ev;
        std::string err;
        if (!parse_events(events, ev, err)) { std::fprintf(stderr, "%s\n", err.c_str()); return 2; }
        pt_viewer* view = nullptr;
        if (pt_viewer_create(cam, mode, &view)) { std::fprintf(stderr, "pt_viewer_create failed\n"); return 1; }
        for (const Event& e : ev) {
            if (e.kind == 1) pt_viewer_key(view, e.key, e.action);
            else if (e.kind == 2) pt_viewer_cursor(view, e.a, e.b);
            else {
                if (pt_viewer_should_close(view)) break;     // glfwWindowShouldClose (:160)
                pt_viewer_frame_info fi;
                pt_viewer_next(view, e.a, &fi);
                for (int g = 0; g < nctx; g++) {
                    CHECK(pt_set_display_mode(ctx[g], fi.display_mode), ctx[g]);
                    CHECK(pt_set_camera(ctx[g], fi.camera), ctx[g]);
                    CHECK(pt_render_async(ctx[g], fi.frame, 1, fi.accumulate), ctx[g]);
                }
                frames_run++;
                resets += fi.accumulate == 0;
            }
        }
        pt_viewer_destroy(view);
        spp = frames_run;
    } else if (until && !use_film) {
        // frames 1.. in batches until the noise summary meets the target (or max_spp frames)
        int done = 0;
        if (adaptive) {     // ... each tile until it meets the target on its own
            CHECK(pt_render_adaptive(ctx[0], 1, 0, batch, max_spp, noise_target, &done, &astats), ctx[0]);
            noise = astats.noise;
            if (!spp_map.empty()) {
                int nt = 0, tx = 1;
                CHECK(pt_read_tile_frames(ctx[0], nullptr, 0, &nt, &tx), ctx[0]);
                std::vector<unsigned> fr((size_t)std::max(nt, 1), 0u);
                CHECK(pt_read_tile_frames(ctx[0], fr.data(), nt, &nt, &tx), ctx[0]);
                unsigned mx = 0;
                for (int t = 0; t < nt; t++) mx = std::max(mx, fr[t]);
                const int ty = tx > 0 ? nt / tx : 0, maxval = mx > 255 ? 65535 : 255;
                FILE* f = std::fopen(spp_map.c_str(), "wb");
                if (!f) { std::fprintf(stderr, "cannot write %s\n", spp_map.c_str()); return 1; }
                std::fprintf(f, "P5\n%d %d\n%d\n", tx, ty, maxval);
                for (int y = ty - 1; y >= 0; y--)        // PGM rows run top-to-bottom: flip (image row 0 = bottom)
                    for (int x = 0; x < tx; x++) {
                        const unsigned v = std::min(fr[(size_t)y * tx + x], 65535u);
                        if (maxval > 255) std::fputc((int)(v >> 8), f);      // 16-bit samples: most significant byte first
                        std::fputc((int)(v & 255u), f);
                    }
                std::fclose(f);
            }
        } else {
            CHECK(pt_render_until(ctx[0], 1, 0, batch, max_spp, noise_target, &done, &noise), ctx[0]);
        }
        spp = done;
    } else if (cam_model >= 0) {
        // frames 1..spp through the camera model, then the image into the context for the reads below
        pcam.model = cam_model, pcam.width = W, pcam.height = H;
        std::memcpy(pcam.cam, cam, sizeof(cam));
        if (focus_at) {
            pt_hit h;
            CHECK(pt_pick(ctx[0], focus_xy, 1, &h), ctx[0]);
            if (h.kind == PT_HIT_NONE) {
                std::fprintf(stderr, "--focus-at %d,%d: nothing under that pixel to focus on\n", focus_xy[0], focus_xy[1]);
                return 1;
            }
            // dot(p - pos, fwd) in binary32: fwd = dir * (1 / sqrt(dot(dir, dir))), dot = (x + y) + z
            const float q = (cam[4] * cam[4] + cam[5] * cam[5]) + cam[6] * cam[6], r = 1.0f / std::sqrt(q);
            const float fx = cam[4] * r, fy = cam[5] * r, fz = cam[6] * r;
            pcam.focus = ((h.p[0] - cam[0]) * fx + (h.p[1] - cam[1]) * fy) + (h.p[2] - cam[2]) * fz;
            std::printf("focus at pixel (%d, %d): %.9g\n", focus_xy[0], focus_xy[1], pcam.focus);
        }
        if (use_film) {
            // ... through a film: the image, the moments and the guides of this camera stay on the device
            CHECK(pt_film_create(ctx[0], &pcam, dparams.guide_frames, &film), ctx[0]);
            if (until) {
                int done = 0;
                CHECK(pt_film_expose_until(film, 1, 0, batch, max_spp, noise_target, &done, &noise), ctx[0]);
                spp = done;
            } else {
                for (int k = 0; k < spp; k += chunk) {
                    const int n = std::min(chunk, spp - k), f0 = 1 + k;
                    CHECK(pt_film_expose(film, f0, n, f0 == 1 ? 0 : 1), ctx[0]);
                }
                if (spp >= 2) CHECK(pt_film_noise(film, 0.0f, &noise), ctx[0]);
            }
        } else {
            std::vector<float> cimg(4 * (size_t)W * H, 0.0f);
            for (int k = 0; k < spp; k += chunk) {
                const int n = std::min(chunk, spp - k), f0 = 1 + k;
                CHECK(pt_trace_camera(ctx[0], &pcam, f0, n, f0 == 1 ? 0 : 1, cimg.data()), ctx[0]);
            }
            CHECK(pt_write_rgba32f(ctx[0], cimg.data(), cimg.size() * 4), ctx[0]);
        }
    } else {
        for (int k = 0; k < spp; k += chunk) {
            const int n = std::min(chunk, spp - k), f0 = first + k;
            // frame 1 after a reset overwrites (accumulate = 0); a resumed run accumulates
            for (int g = 0; g < nctx; g++) CHECK(pt_render_async(ctx[g], f0, n, f0 == 1 ? 0 : 1), ctx[g]);
        }
    }
    std::vector<float> img(4 * (size_t)W * H, 0.0f);
    double gather_ms = 0.0;
    if (group) {      // stream-ordered after every context's renders: the gather is the sync
        int grc = pt_group_gather_rgba32f(group, img.data(), img.size() * 4, 0);
        if (grc) { std::fprintf(stderr, "pt_group_gather_rgba32f: %s (%d)\n", pt_group_last_error(group), grc); return 1; }
        pt_group_stats(group, &gather_ms, nullptr);
    }
    for (int g = 0; g < nctx; g++) CHECK(pt_sync(ctx[g]), ctx[g]);
    double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count();
    if (events) std::printf("replayed %s: %d frames, %d accumulation restarts\n", events, frames_run, resets);

    std::vector<unsigned char> rgba(4 * (size_t)W * H, 0);
    if (group) {      // the ACES view of the gathered frame, tonemapped on the root device
        int grc = pt_group_gather_rgba8_aces(group, rgba.data(), rgba.size(), 0);
        if (grc) { std::fprintf(stderr, "pt_group_gather_rgba8_aces: %s (%d)\n", pt_group_last_error(group), grc); return 1; }
    }
    for (int g = 0; g < nctx && !group; g++) {     // one context: its own ACES view and rows
        int rows = 0, r0 = 0, rs = 1;
        pt_rows(ctx[g], &rows, &r0, &rs);
        std::vector<unsigned char> part8(4 * (size_t)rows * W);
        CHECK(pt_read_rgba8_aces(ctx[g], part8.data(), part8.size()), ctx[g]);
        CHECK(pt_read_rgba32f(ctx[g], img.data(), img.size() * 4), ctx[g]);
        for (int k = 0; k < rows; k++)
            std::memcpy(&rgba[4 * (size_t)(r0 + k * rs) * W], &part8[4 * (size_t)k * W], 4 * (size_t)W);
    }
    std::vector<float> dimg;
    std::vector<unsigned char> drgba;
    if (film) {       // the film's planes, not the context's image
        CHECK(pt_film_read(film, PT_FILM_IMAGE, img.data(), img.size() * 4), ctx[0]);
        CHECK(pt_film_read(film, PT_FILM_IMAGE_ACES8, rgba.data(), rgba.size()), ctx[0]);
        if (denoise) {
            auto td = std::chrono::steady_clock::now();
            CHECK(pt_film_denoise(film, &dparams, &dinfo), ctx[0]);
            dimg.assign(4 * (size_t)W * H, 0.0f);
            drgba.assign(4 * (size_t)W * H, 0);
            CHECK(pt_film_read(film, PT_FILM_DENOISED, dimg.data(), dimg.size() * 4), ctx[0]);
            denoise_ms = std::chrono::duration<double>(std::chrono::steady_clock::now() - td).count() * 1e3;
            CHECK(pt_film_read(film, PT_FILM_DENOISED_ACES8, drgba.data(), drgba.size()), ctx[0]);
        }
        CHECK(pt_film_info(film, &film_frames, &film_held), ctx[0]);
        pt_film_destroy(film);
    } else if (denoise) {    // the filtered view of the finished image (the image itself stays as rendered)
        auto td = std::chrono::steady_clock::now();
        CHECK(pt_denoise(ctx[0], &dparams, &dinfo), ctx[0]);
        denoise_ms = std::chrono::duration<double>(std::chrono::steady_clock::now() - td).count() * 1e3;
        dimg.assign(4 * (size_t)W * H, 0.0f);
        drgba.assign(4 * (size_t)W * H, 0);
        CHECK(pt_read_denoised_rgba32f(ctx[0], dimg.data(), dimg.size() * 4), ctx[0]);
        CHECK(pt_read_denoised_rgba8_aces(ctx[0], drgba.data(), drgba.size()), ctx[0]);
    }
    if (queries && run_queries()) return 1;
    pt_group_destroy(group);
    for (int g = 0; g < nctx; g++) pt_destroy(ctx[g]);
    std::printf("rendered %dx%d, %d spp, %d bounces on %d GPU(s), %d context(s): %.3f s, %.3f ms/frame\n", W, H, spp,
                bounces, gpus, nctx, secs, secs * 1e3 / (spp > 0 ? spp : 1));
    if (group) std::printf("RCCL gather: %.3f ms\n", gather_ms);
    if (!checkpoint.empty()) {
        if (!save_checkpoint(checkpoint, W, H, first + spp, key, img)) {
            std::fprintf(stderr, "cannot write checkpoint %s\n", checkpoint.c_str());
            return 1;
        }
    }
    const double npx = noise.pixels ? (double)noise.pixels : 1.0;
    if (until)
        std::printf("noise target %g: %d frames, mean relative error %.5f, max %.5f, %.2f%% of pixels above\n",
                    noise_target, spp, (double)noise.sum_q / npx / 65536.0, noise.max_q / 65536.0,
                    100.0 * (double)noise.above / npx);
    if (json) {
        std::printf("{\"width\": %d, \"height\": %d, \"frames\": %d, \"first_frame\": %d, \"bounces\": %d, "
                    "\"gpus\": %d, \"contexts\": %d, \"seconds\": %.6f, \"ms_per_frame\": %.4f, \"triangles\": %d, "
                    "\"nodes\": %d, \"gather_ms\": %.4f",
                    W, H, spp, first, bounces, gpus, nctx, secs, secs * 1e3 / (spp > 0 ? spp : 1), cnt[0], cnt[3],
                    gather_ms);
        if (until)
            std::printf(", \"frames_done\": %d, \"noise_mean\": %.8f, \"noise_max\": %.8f, \"noise_above_frac\": %.8f",
                        spp, (double)noise.sum_q / npx / 65536.0, noise.max_q / 65536.0, (double)noise.above / npx);
        if (use_film) {
            std::printf(", \"film\": {\"frames\": %d, \"guides_held\": %d", film_frames, film_held);
            if (film_frames >= 2)
                std::printf(", \"noise_mean\": %.8f, \"noise_max\": %.8f, \"sum_q\": %llu, \"pixels\": %llu",
                            (double)noise.sum_q / npx / 65536.0, noise.max_q / 65536.0, noise.sum_q, noise.pixels);
            std::printf("}");
        }
        if (adaptive)
            std::printf(", \"tiles\": %llu, \"tiles_active\": %llu, \"pixel_frames\": %llu", astats.tiles,
                        astats.tiles_active, astats.pixel_frames);
        if (denoise)
            std::printf(", \"denoise\": {\"guided\": %d, \"guides_rendered\": %d, \"iterations\": %d, "
                        "\"guide_frames\": %d, \"frames\": %d, \"ms\": %.4f}",
                        dinfo.guided, dinfo.guides_rendered, dinfo.iterations, dparams.guide_frames, dinfo.frames, denoise_ms);
        std::printf("}\n");
    }
    if (denoise && !denoise_pfm.empty()) {
        FILE* f = std::fopen(denoise_pfm.c_str(), "wb");
        if (!f) { std::fprintf(stderr, "cannot write %s\n", denoise_pfm.c_str()); return 1; }
        std::fprintf(f, "PF\n%d %d\n-1.0\n", W, H);
        for (size_t i = 0; i < (size_t)W * H; i++) std::fwrite(&dimg[4 * i], 4, 3, f);
        std::fclose(f);
    }
    if (denoise && !denoise_ppm.empty()) {
        FILE* f = std::fopen(denoise_ppm.c_str(), "wb");
        if (!f) { std::fprintf(stderr, "cannot write %s\n", denoise_ppm.c_str()); return 1; }
        std::fprintf(f, "P6\n%d %d\n255\n", W, H);
        for (int y = H - 1; y >= 0; y--)
            for (int x = 0; x < W; x++) std::fwrite(&drgba[4 * ((size_t)y * W + x)], 1, 3, f);
        std::fclose(f);
    }

    if (FILE* f = std::fopen(pfm.c_str(), "wb")) {       // PFM rows run bottom-to-top: no flip
        std::fprintf(f, "PF\n%d %d\n-1.0\n", W, H);
        for (size_t i = 0; i < (size_t)W * H; i++) std::fwrite(&img[4 * i], 4, 3, f);
        std::fclose(f);
    }
    if (FILE* f = std::fopen(ppm.c_str(), "wb")) {       // PPM rows run top-to-bottom: flip
        std::fprintf(f, "P6\n%d %d\n255\n", W, H);
        for (int y = H - 1; y >= 0; y--)
            for (int x = 0; x < W; x++) std::fwrite(&rgba[4 * ((size_t)y * W + x)], 1, 3, f);
        std::fclose(f);
    }
    return 0;
}
