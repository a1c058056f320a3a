// cli.cpp — headless counterpart of RTBase's Main.cpp (RTBase/Main.cpp:14-150) on librth + librtg.
//
// Same arguments and stopping rule as the reference's frame loop:
//   -scene <dir>  -SPP <n>  -outputFilename <file>
// frames of +1 spp until SPP is reached or 10 s of render time have passed, then the film is
// written as result_<spp>.hdr (Film::save). The window / camera keys have no headless meaning;
// 'P' and 'L' (saveHDR / savePNG of -outputFilename) become: -outputFilename is always written at
// the end, as .hdr or, for a .png name, tonemapped PNG (RayTracer::savePNG).
// Extra options (defaults keep the reference behaviour): -width -height (override scene.json),
// -maxDepth (MAX_DEPTH, 4), -seed (sampler seed, 1234), -device, -batch (spp per render call;
// results do not depend on it), -sync 1 (wait for every frame; default: frames are queued with
// rtg_render_async and up to three run side by side, the film is read once at the end),
// -skipMissing 1 (filtered scene variants), -envmap <file>, -timeLimit <s> (10; 0 = none).
// "Frame time" is the wall time of each render call, as Main.cpp:113-117 times rt.render(); with
// queued frames a call returns once the frame three before it has left the GPU, so in the steady
// state it is the GPU's time per frame.
// -denoise 1 additionally writes the denoised film (rtg_denoise: the project's own edge-avoiding
// a-trous wavelet filter guided by albedo and normals, standing in for the reference's never-called
// OIDN pass) as RGBE next to the normal output, with _denoised before the extension
// (-outputFilename's name when given, else result_<spp>); optional -denoiseIterations (5),
// -denoiseSigmaColour (1), -denoiseSigmaAlbedo (0.1). The normal output is unchanged. With -gpus /
// -devices it goes through rtg_group_denoise.
// Anti-aliasing and depth of field (rtg_set_camera_sampling, include/rtg.h): -pixelFilter none|box|tent
// (none: every sample through the pixel centre, the reference's renderTile), -filterRadius r (pixels;
// default 0.5 for box, 1 for tent), -lensRadius R (0: pinhole) and -focalDistance f, for one device
// and for -gpus / -devices alike.
// Environment light sampling (rtg_set_env_sampling): -envSampling uniform|luminance (uniform: the
// reference's EnvironmentMap::sample; luminance: NEE directions drawn in proportion to the map's
// luminance through an alias table), for one device and for -gpus / -devices alike.
// Light selection for NEE (rtg_set_light_sampling): -lightSampling uniform|power (uniform: the
// reference's Scene::sampleLight; power: lights picked by emitted power through an alias table) and
// -lightUniformShare x (the share of the uniform pick mixed in, default 0.125), for one device and for
// -gpus / -devices alike. -lightGrid N (default 0, off; with -lightSampling power): the pick comes from
// the alias table of the grid cell that holds the shading point, N cells on the scene's longest axis
// (rtg_set_light_grid).
// Material model (rtg_set_material_model): -materials reference|physical (reference: conductor, plastic
// and Oren-Nayar materials shade as the reference's Lambertian stubs; physical: GGX conductor, coated
// plastic and Oren-Nayar from the scene's own roughness, eta, k, IORs and alpha), for one device and for
// -gpus / -devices alike. -transmission 0|1 (default 0; needs -materials physical): 1 shades the scene's
// rough dielectrics with GGX reflection and refraction (rth_scene_material_params_transmissive) instead
// of the Lambertian stub.
// Path-tracer MIS (rtg_set_path_mis): -pathMIS off|power (off: the reference's pathTrace; power: NEE and
// BSDF-sampled emitter hits combined with the power heuristic, a miss weighted by the throughput), for one
// device and for -gpus / -devices alike.
// Sampler (rtg_set_sampler): -sampler pcg|sobol (pcg: one PCG32 stream per pixel and sample; sobol: an
// Owen-scrambled Sobol sequence over the samples of a pixel, four dimensions per bounce), for one device
// and for -gpus / -devices alike.
// Camera pose (rtg_set_camera): -from "x y z" -to "x y z" -up "x y z" -fov degrees override scene.json's
// pose through rth_camera_look_at, the loader's own camera code; each is optional and keeps the scene's
// value when absent. For one device and for -gpus / -devices alike.
// AOVs (rtg_gbuffer): -aov PREFIX writes, after the render, PREFIX_albedo.hdr, PREFIX_normal.hdr (the
// denoiser's guides: first-hit albedo and |shading normal|) and PREFIX_depth.hdr (the first hit's distance t in
// all three channels, 0 on a miss) as RGBE, from one traversal of the pixel-centre camera rays; with -from / -to
// / -up / -fov they are the AOVs of that pose. One device only.
// Frame loop with poses (Main.cpp:74-118 with a camera that moves; rtg_svgf_accumulate): -orbit "N DEG" runs N
// poses on an arc of DEG degrees about the centre of the scene's bounds (axis: the up vector), starting at the
// scene's (or -from's) position and looking at that centre (tests/temporal_ref.py: orbit, in binary64). Per pose i:
// rtg_set_camera, rtg_clear, -SPP samples under seed + i, then rtg_svgf_accumulate, or with -svgfIllum 1
// rtg_svgf_illum_accumulate. -svgfPlaneTolerance x sets plane_tolerance (default 0.01). The last
// pose's film is written as above, the filtered image of the last pose as <name>_svgf.hdr (<name> as for
// _denoised). No time limit. One device only.
// Multi-GPU (one node): -gpus N renders on devices 0..N-1, -devices a,b,... on a list. Rank r
// renders the 32x32 tiles with (tile_x + tile_y) % N == r, and the film is assembled on the first
// device from every device's own tiles (packed, one RCCL send per device, scattered) before it is
// written (rtg_group_*, include/rtg.h); the output is bit-identical to the one-device render. Frames
// are queued on every device (rtg_group_render_async: coalesced and pipelined per device, as on one
// device) unless -sync 1 (rtg_group_render: each call waits for every device).
#include "../../../include/rth.h"

#include <chrono>
#include <cmath>
#include <cstdio>
#include <sstream>
#include <cstdlib>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

static int die(const char* what, const char* msg) {
    std::fprintf(stderr, "rtg_render: %s: %s\n", what, msg ? msg : "");
    return 1;
}

int main(int argc, char** argv) {
    std::string scene_name = "MaterialsScene", filename = "GI.hdr";
    unsigned spp_target = 8192;
    std::unordered_map<std::string, std::string> args;
    for (int i = 1; i < argc; ++i) {
        std::string a = argv[i];
        if (!a.empty() && a[0] == '-') {
            if (i + 1 < argc) args[a] = argv[++i];
            else std::fprintf(stderr, "Error: Missing value for argument '%s'\n", a.c_str());
        } else {
            std::fprintf(stderr, "Warning: Ignoring unexpected argument '%s'\n", a.c_str());
        }
    }
    auto get = [&](const char* k, const std::string& d) { auto it = args.find(k); return it == args.end() ? d : it->second; };
    scene_name = get("-scene", scene_name);
    filename = get("-outputFilename", filename);
    spp_target = (unsigned)std::stoul(get("-SPP", std::to_string(spp_target)));
    const bool out_given = args.count("-outputFilename") > 0;
    rth_load_options lo{};
    lo.width = std::stoi(get("-width", "0"));
    lo.height = std::stoi(get("-height", "0"));
    lo.skip_missing = std::stoi(get("-skipMissing", "0"));
    std::string env = get("-envmap", "");
    lo.envmap = env.empty() ? nullptr : env.c_str();
    const int max_depth = std::stoi(get("-maxDepth", "4"));
    const uint64_t seed = std::stoull(get("-seed", "1234"));
    const int device = std::stoi(get("-device", "0"));
    const unsigned batch = (unsigned)std::max(1, std::stoi(get("-batch", "1")));
    const double time_limit = std::stod(get("-timeLimit", "10"));
    const bool sync = std::stoi(get("-sync", "0")) != 0;

    rth_scene* scene = nullptr;
    if (rth_load_scene(scene_name.c_str(), &lo, &scene) != 0) return die("loadScene", rth_last_error());
    rth_scene_info info{};
    rth_scene_get_info(scene, &info);
    std::vector<int> devices;
    if (args.count("-devices")) {
        std::stringstream ss(args["-devices"]);
        std::string tok;
        while (std::getline(ss, tok, ',')) devices.push_back(std::stoi(tok));
    } else if (args.count("-gpus")) {
        for (int i = 0; i < std::stoi(args["-gpus"]); ++i) devices.push_back(i);
    }
    // -pixelFilter none|box|tent -filterRadius r -lensRadius R -focalDistance f (rtg_set_camera_sampling)
    rtg_camera_sampling cs{};
    rtg_camera_sampling_defaults(&cs);
    const std::string pf = get("-pixelFilter", "none");
    if (pf == "none") cs.filter = RTG_FILTER_NONE;
    else if (pf == "box") cs.filter = RTG_FILTER_BOX;
    else if (pf == "tent") cs.filter = RTG_FILTER_TENT;
    else return die("-pixelFilter", "one of none, box, tent");
    cs.filter_radius = std::stof(get("-filterRadius", cs.filter == RTG_FILTER_TENT ? "1" : "0.5"));
    cs.lens_radius = std::stof(get("-lensRadius", "0"));
    cs.focal_distance = std::stof(get("-focalDistance", "1"));
    const std::string es = get("-envSampling", "uniform");
    if (es != "uniform" && es != "luminance") return die("-envSampling", "one of uniform, luminance");
    const int env_mode = es == "luminance" ? RTG_ENV_LUMINANCE : RTG_ENV_UNIFORM;
    rtg_light_sampling lsm{};
    rtg_light_sampling_defaults(&lsm);
    const std::string lsn = get("-lightSampling", "uniform");
    if (lsn != "uniform" && lsn != "power") return die("-lightSampling", "one of uniform, power");
    lsm.mode = lsn == "power" ? RTG_LIGHTS_POWER : RTG_LIGHTS_UNIFORM;
    lsm.uniform_share = std::stof(get("-lightUniformShare", "0.125"));
    rtg_light_grid lgr{};
    rtg_light_grid_defaults(&lgr);
    const int lgn = std::stoi(get("-lightGrid", "0"));
    if (lgn < 0) return die("-lightGrid", "0 (off) or the number of cells on the longest axis");
    lgr.cells = (uint32_t)lgn;
    const std::string mtl = get("-materials", "reference");
    if (mtl != "reference" && mtl != "physical") return die("-materials", "one of reference, physical");
    const bool physical = mtl == "physical";
    const std::string trn = get("-transmission", "0");
    if (trn != "0" && trn != "1") return die("-transmission", "one of 0, 1");
    if (trn == "1" && !physical) return die("-transmission", "needs -materials physical");
    const std::string pmn = get("-pathMIS", "off");
    if (pmn != "off" && pmn != "power") return die("-pathMIS", "one of off, power");
    const int path_mis = pmn == "power" ? RTG_PATH_MIS_POWER : RTG_PATH_MIS_OFF;
    const std::string smn = get("-sampler", "pcg");
    if (smn != "pcg" && smn != "sobol") return die("-sampler", "one of pcg, sobol");
    const int sampler = smn == "sobol" ? RTG_SAMPLER_SOBOL : RTG_SAMPLER_PCG;
    uint32_t n_params = 0;
    const rtg_material_params* params = trn == "1" ? rth_scene_material_params_transmissive(scene, &n_params)
                                                   : rth_scene_material_params(scene, &n_params);
    // -from / -to / -up / -fov: the scene's pose with the given parts replaced (rth_camera_look_at)
    const bool pose_given = args.count("-from") || args.count("-to") || args.count("-up") || args.count("-fov");
    rtg_camera new_cam{};
    rtg_camera_proj new_proj{};
    if (pose_given) {
        float from[3], to[3], up[3], fov = 0.0f;
        int32_t flip_x = 0;
        if (rth_scene_camera_pose(scene, from, to, up, &fov, &flip_x) != 0) return die("camera pose", rth_last_error());
        auto vec3 = [&](const char* k, float* v) {
            if (!args.count(k)) return true;
            std::stringstream ss(args[k]);
            float t[3];
            std::string rest;
            if (!(ss >> t[0] >> t[1] >> t[2]) || (ss >> rest)) return false;
            v[0] = t[0]; v[1] = t[1]; v[2] = t[2];
            return true;
        };
        if (!vec3("-from", from)) return die("-from", "three numbers, as \"x y z\"");
        if (!vec3("-to", to)) return die("-to", "three numbers, as \"x y z\"");
        if (!vec3("-up", up)) return die("-up", "three numbers, as \"x y z\"");
        if (args.count("-fov")) fov = std::stof(args["-fov"]);
        if (rth_camera_look_at(from, to, up, fov, info.width, info.height, flip_x, &new_cam, &new_proj) != 0)
            return die("rth_camera_look_at", rth_last_error());
    }
    const std::string aov = get("-aov", "");
    if (!aov.empty() && !devices.empty()) return die("-aov", "one device only (not with -gpus / -devices)");
    // -orbit "N DEG": the poses of the frame loop (temporal_ref.orbit)
    std::vector<std::pair<rtg_camera, rtg_camera_proj>> orbit;
    if (args.count("-orbit")) {
        if (!devices.empty()) return die("-orbit", "one device only (not with -gpus / -devices)");
        std::stringstream os(args["-orbit"]);
        int n_poses = 0;
        double total_deg = 0.0;
        std::string rest;
        if (!(os >> n_poses >> total_deg) || (os >> rest) || n_poses < 1) return die("-orbit", "a count and an angle, as \"N DEG\"");
        float from[3], to[3], up[3], fov = 0.0f;
        int32_t flip_x = 0;
        if (rth_scene_camera_pose(scene, from, to, up, &fov, &flip_x) != 0) return die("camera pose", rth_last_error());
        auto vec3 = [&](const char* k, float* v) {
            if (!args.count(k)) return true;
            std::stringstream ss(args[k]);
            return bool(ss >> v[0] >> v[1] >> v[2]);
        };
        if (!vec3("-from", from) || !vec3("-up", up)) return die("-orbit", "-from and -up take three numbers");
        if (args.count("-fov")) fov = std::stof(args["-fov"]);
        double c[3], v[3], k[3];
        for (int a = 0; a < 3; ++a) {
            c[a] = 0.5 * ((double)info.bounds_min[a] + (double)info.bounds_max[a]);
            v[a] = (double)from[a] - c[a];
            k[a] = up[a];
        }
        const double kl = std::sqrt((k[0] * k[0] + k[1] * k[1]) + k[2] * k[2]);
        for (double& x : k) x /= kl;
        const double kv = (k[0] * v[0] + k[1] * v[1]) + k[2] * v[2];
        const double cr[3] = {k[1] * v[2] - k[2] * v[1], k[2] * v[0] - k[0] * v[2], k[0] * v[1] - k[1] * v[0]};
        for (int i = 0; i < n_poses; ++i) {  // Rodrigues' rotation of from - c about up
            const double ang = (total_deg * i / std::max(n_poses - 1, 1)) * (M_PI / 180.0);
            float f[3], t[3];
            for (int a = 0; a < 3; ++a) {
                f[a] = (float)(c[a] + ((v[a] * std::cos(ang) + cr[a] * std::sin(ang)) + k[a] * kv * (1 - std::cos(ang))));
                t[a] = (float)c[a];
            }
            rtg_camera oc{};
            rtg_camera_proj op{};
            if (rth_camera_look_at(f, t, up, fov, info.width, info.height, flip_x, &oc, &op) != 0)
                return die("rth_camera_look_at", rth_last_error());
            orbit.emplace_back(oc, op);
        }
    }
    rtg_handle* rt = nullptr;
    rtg_group* grp = nullptr;
    if (devices.empty()) {
        if (rtg_create(device, rth_scene_desc(scene), &rt) != 0) return die("rtg_create", rtg_last_error());
        if (rtg_set_options(rt, max_depth, RTG_OPT_CULL, 0) != 0) return die("rtg_set_options", rtg_last_error());
        if (rtg_set_camera_sampling(rt, &cs) != 0) return die("rtg_set_camera_sampling", rtg_last_error());
        if (rtg_set_env_sampling(rt, env_mode) != 0) return die("rtg_set_env_sampling", rtg_last_error());
        if (rtg_set_light_sampling(rt, &lsm) != 0) return die("rtg_set_light_sampling", rtg_last_error());
        if (rtg_set_light_grid(rt, &lgr) != 0) return die("rtg_set_light_grid", rtg_last_error());
        if (physical && (rtg_set_material_params(rt, params, n_params) != 0 ||
                         rtg_set_material_model(rt, RTG_MATERIALS_PHYSICAL) != 0))
            return die("rtg_set_material_model", rtg_last_error());
        if (rtg_set_path_mis(rt, path_mis) != 0) return die("rtg_set_path_mis", rtg_last_error());
        if (rtg_set_sampler(rt, sampler) != 0) return die("rtg_set_sampler", rtg_last_error());
        if (pose_given && rtg_set_camera(rt, &new_cam, &new_proj) != 0) return die("rtg_set_camera", rtg_last_error());
    } else {
        if (rtg_group_create(devices.data(), (int)devices.size(), rth_scene_desc(scene), &grp) != 0)
            return die("rtg_group_create", rtg_last_error());
        if (rtg_group_set_options(grp, max_depth, RTG_OPT_CULL, 0) != 0) return die("rtg_group_set_options", rtg_last_error());
        if (rtg_group_set_camera_sampling(grp, &cs) != 0) return die("rtg_group_set_camera_sampling", rtg_last_error());
        if (rtg_group_set_env_sampling(grp, env_mode) != 0) return die("rtg_group_set_env_sampling", rtg_last_error());
        if (rtg_group_set_light_sampling(grp, &lsm) != 0) return die("rtg_group_set_light_sampling", rtg_last_error());
        if (rtg_group_set_light_grid(grp, &lgr) != 0) return die("rtg_group_set_light_grid", rtg_last_error());
        if (physical && (rtg_group_set_material_params(grp, params, n_params) != 0 ||
                         rtg_group_set_material_model(grp, RTG_MATERIALS_PHYSICAL) != 0))
            return die("rtg_group_set_material_model", rtg_last_error());
        if (rtg_group_set_path_mis(grp, path_mis) != 0) return die("rtg_group_set_path_mis", rtg_last_error());
        if (rtg_group_set_sampler(grp, sampler) != 0) return die("rtg_group_set_sampler", rtg_last_error());
        if (pose_given && rtg_group_set_camera(grp, &new_cam, &new_proj) != 0)
            return die("rtg_group_set_camera", rtg_last_error());
        std::printf("%d devices, own-tile film exchange by %s\n", (int)devices.size(),
                    rtg_group_uses_rccl(grp) ? "RCCL (ncclSend/ncclRecv)"
                    : devices.size() == 1    ? "none (one device)"
                                             : "device copies (repeated devices)");
    }
    std::printf("scene %s: %u triangles, %u lights, %dx%d (load %.0f ms, BVH %.0f ms)\n", scene_name.c_str(),
                info.n_tris, info.n_lights, info.width, info.height, info.load_ms, info.bvh_ms);

    unsigned spp = 0;
    double total = 0.0;
    const auto w0 = std::chrono::steady_clock::now();
    std::vector<float> filtered;
    if (!orbit.empty()) {  // the frame loop with poses: move, clear, render, filter
        const bool illum = std::stoi(get("-svgfIllum", "0")) != 0;
        rtg_svgf_illum_params ip{};
        rtg_svgf_illum_defaults(&ip);
        ip.svgf.temporal.plane_tolerance = std::stof(get("-svgfPlaneTolerance", std::to_string(ip.svgf.temporal.plane_tolerance)));
        filtered.resize((size_t)info.width * info.height * 3);
        for (size_t i = 0; i < orbit.size(); ++i) {
            auto t0 = std::chrono::steady_clock::now();
            if (rtg_set_camera(rt, &orbit[i].first, &orbit[i].second) != 0) return die("rtg_set_camera", rtg_last_error());
            if (rtg_clear(rt) != 0) return die("rtg_clear", rtg_last_error());
            if (rtg_render(rt, 0, spp_target, seed + i, nullptr, 0) != 0) return die("rtg_render", rtg_last_error());
            if ((illum ? rtg_svgf_illum_accumulate(rt, &ip, filtered.data())
                       : rtg_svgf_accumulate(rt, &ip.svgf, filtered.data())) != 0)
                return die(illum ? "rtg_svgf_illum_accumulate" : "rtg_svgf_accumulate", rtg_last_error());
            const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            total += dt;
            std::printf("Pose %zu | Frame time: %gs | Total time: %gs\n", i, dt, total);
        }
        spp = spp_target;
    }
    while (spp < spp_target) {
        const unsigned n = std::min(batch, spp_target - spp);
        auto t0 = std::chrono::steady_clock::now();
        const int rc = grp    ? (sync ? rtg_group_render(grp, spp, n, seed) : rtg_group_render_async(grp, spp, n, seed))
                       : sync ? rtg_render(rt, spp, n, seed, nullptr, 0)
                              : rtg_render_async(rt, spp, n, seed, nullptr, 0, nullptr);
        if (rc != 0) return die("rtg_render", rtg_last_error());
        const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        total += dt;
        spp += n;
        std::printf("Frame time: %gs | Total time: %gs\nSPP: %u\n", dt, total, spp);
        if (time_limit > 0 && total >= time_limit) break;
    }
    std::vector<float> film((size_t)info.width * info.height * 3);
    uint32_t got = 0;
    if (rt && rtg_synchronize(rt) != 0) return die("rtg_synchronize", rtg_last_error());
    if (grp && rtg_group_synchronize(grp) != 0) return die("rtg_group_synchronize", rtg_last_error());
    const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - w0).count();
    std::printf("%u spp in %.4f s of wall time (%s): %.4f ms per spp, %.1f Mpaths/s\n", spp, wall,
                grp ? (sync ? "device group, synchronous calls" : "device group, queued calls")
                    : sync ? "synchronous calls" : "queued calls", 1e3 * wall / std::max(1u, spp),
                (double)spp * info.width * info.height / wall / 1e6);
    if (grp) {
        if (rtg_group_film_read(grp, film.data(), &got) != 0) return die("rtg_group_film_read", rtg_last_error());
        std::printf("film exchange: %.3f ms\n", rtg_group_reduce_ms(grp));
    } else if (rtg_film_read(rt, film.data(), &got) != 0) {
        return die("rtg_film_read", rtg_last_error());
    }
    const std::string auto_name = "result_" + std::to_string(got) + ".hdr";
    if (rth_save_hdr(auto_name.c_str(), info.width, info.height, film.data(), got) != 0)
        return die("saveHDR", rth_last_error());
    std::printf("wrote %s\n", auto_name.c_str());
    if (out_given) {
        const bool png = filename.size() > 4 && filename.compare(filename.size() - 4, 4, ".png") == 0;
        int rc = png ? rth_save_png(filename.c_str(), info.width, info.height, film.data(), got)
                     : rth_save_hdr(filename.c_str(), info.width, info.height, film.data(), got);
        if (rc != 0) return die(png ? "savePNG" : "saveHDR", rth_last_error());
        std::printf("wrote %s\n", filename.c_str());
    }
    if (std::stoi(get("-denoise", "0")) != 0) {
        rtg_denoise_params dp{};
        rtg_denoise_defaults(&dp);
        dp.iterations = (uint32_t)std::stoul(get("-denoiseIterations", std::to_string(dp.iterations)));
        dp.sigma_colour = std::stof(get("-denoiseSigmaColour", std::to_string(dp.sigma_colour)));
        dp.sigma_albedo = std::stof(get("-denoiseSigmaAlbedo", std::to_string(dp.sigma_albedo)));
        std::vector<float> den(film.size());
        if ((grp ? rtg_group_denoise(grp, &dp, den.data()) : rtg_denoise(rt, &dp, den.data())) != 0)
            return die("rtg_denoise", rtg_last_error());
        std::string base = out_given ? filename : auto_name;
        const size_t dot = base.find_last_of('.'), slash = base.find_last_of('/');
        if (dot != std::string::npos && (slash == std::string::npos || dot > slash)) base.erase(dot);
        const std::string den_name = base + "_denoised.hdr";
        if (rth_save_hdr(den_name.c_str(), info.width, info.height, den.data(), 1) != 0)  // already a mean
            return die("saveHDR", rth_last_error());
        std::printf("wrote %s\n", den_name.c_str());
    }
    if (!filtered.empty()) {
        std::string base = out_given ? filename : auto_name;
        const size_t dot = base.find_last_of('.'), slash = base.find_last_of('/');
        if (dot != std::string::npos && (slash == std::string::npos || dot > slash)) base.erase(dot);
        const std::string name = base + "_svgf.hdr";
        if (rth_save_hdr(name.c_str(), info.width, info.height, filtered.data(), 1) != 0)  // already a mean
            return die("saveHDR", rth_last_error());
        std::printf("wrote %s\n", name.c_str());
    }
    if (!aov.empty()) {
        const size_t n = (size_t)info.width * info.height;
        std::vector<float> pos_t(n * 4), alb(n * 3), nrm(n * 3), depth(n * 3);
        if (rtg_gbuffer(rt, pos_t.data(), nullptr, alb.data(), nrm.data()) != 0) return die("rtg_gbuffer", rtg_last_error());
        for (size_t i = 0; i < n; ++i) {
            const float t = pos_t[4 * i + 3];
            depth[3 * i] = depth[3 * i + 1] = depth[3 * i + 2] = t < 3.40282347e+38f ? t : 0.0f;
        }
        const std::pair<const char*, const float*> outs[3] = {{"_albedo.hdr", alb.data()}, {"_normal.hdr", nrm.data()},
                                                              {"_depth.hdr", depth.data()}};
        for (const auto& o : outs) {
            const std::string name = aov + o.first;
            if (rth_save_hdr(name.c_str(), info.width, info.height, o.second, 1) != 0)  // values, not sums
                return die("saveHDR", rth_last_error());
            std::printf("wrote %s\n", name.c_str());
        }
    }
    if (rt) rtg_destroy(rt);
    if (grp) rtg_group_destroy(grp);
    rth_free_scene(scene);
    return 0;
}
