/*
 * rth.h — C-ABI of the host scene front-end (librth.so), the part of RTBase that stays on the
 * CPU above the rtg boundary:
 *
 *   loadScene / loadInstance        RTBase/SceneLoader.h:104-291  -> rth_load_scene()
 *   GEMScene / GEMModelLoader       RTBase/GEMLoader.h:218-750    (scene.json + .gem parsing)
 *   Texture::load                   RTBase/Imaging.h:32-71        (PNG / Radiance .hdr decode)
 *   Scene::init / Scene::build      RTBase/Scene.h:82-106,142-160 (BVH build, light list)
 *   Film::save                      RTBase/Imaging.h:262-271      -> rth_save_hdr()
 *   Film::tonemap + savePNG         RTBase/Imaging.h:233-242, Renderer.h:895-898 -> rth_tonemap(), rth_save_png()
 *
 * It produces the flattened rtg_scene_desc consumed by rtg_create (include/rtg.h).
 */
#ifndef RTH_H
#define RTH_H

#include "rtg.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rth_scene rth_scene;

typedef struct rth_load_options {
    int32_t width;          /* >0: override scene.json "width" before P is built (0 = keep)   */
    int32_t height;         /* >0: override scene.json "height" before P is built (0 = keep)  */
    int32_t skip_missing;   /* 1: drop instances whose .gem or reflectance file is missing    */
                            /*    (the "_f" filtered variants); 0: error    */
    int32_t bvh_threads;    /* host threads for the BVH build (0 = hardware concurrency)      */
    const char* envmap;     /* non-NULL: override scene.json "envmap" (file in the scene dir) */
} rth_load_options;

typedef struct rth_scene_info {
    uint32_t n_tris, n_nodes, n_materials, n_textures, n_lights, bvh_depth;
    int32_t width, height;
    int32_t env_in_lights;
    uint32_t dropped_instances;   /* instances skipped by skip_missing                      */
    double load_ms, bvh_ms;       /* wall time of parsing+transform and of Scene::build     */
    float bounds_min[3], bounds_max[3];
} rth_scene_info;

const char* rth_last_error(void);
/* Hash of the sources, headers and compile flags this library was built from (build.py). */
const char* rth_build_id(void);

int  rth_load_scene(const char* scene_dir, const rth_load_options* opts, rth_scene** out);
void rth_free_scene(rth_scene* s);
const rtg_scene_desc* rth_scene_desc(const rth_scene* s);
int  rth_scene_get_info(const rth_scene* s, rth_scene_info* out);
/* Index (pre-build load order) of each post-build triangle: the BVH permutation. */
int  rth_scene_permutation(const rth_scene* s, uint32_t* out /* n_tris */);
/* What SceneLoader.h:117-171 hands the BSDF constructors, one record per rtg_scene_desc.materials entry
 * in that order (include/rtg.h: rtg_set_material_params): conductor eta, k and alpha = 1.62142f *
 * sqrtf(roughness); plastic intIOR, extIOR and alpha; orennayar sigma, read from the key "alpha"; with
 * the loader's defaults (roughness 1, intIOR 1.33, extIOR 1, alpha 1, eta and k 0). The rough dielectric
 * keeps intIOR, extIOR and alpha under the tag RTG_MODEL_REFERENCE (no model uses them); every other bsdf:
 * RTG_MODEL_REFERENCE, all parameters 0. The pointer lives as long as the scene. */
const rtg_material_params* rth_scene_material_params(const rth_scene* s, uint32_t* n /* or NULL */);
/* The same records with the loader's rough dielectrics ("bsdf": "dielectric" with roughness >= 0.001, kind
 * RTG_MAT_LAMBERT) tagged RTG_MODEL_ROUGH_DIELECTRIC: what rtg_set_material_params takes for rough
 * dielectric transmission (include/rtg.h). Every other record equals rth_scene_material_params' field
 * for field. */
const rtg_material_params* rth_scene_material_params_transmissive(const rth_scene* s, uint32_t* n /* or NULL */);

/* The camera of loadScene (SceneLoader.h:242-260) from a pose: the code rth_load_scene itself runs on
 * scene.json's "from", "to", "up", "fov" and "flipX" (Matrix::perspective(0.001f, 10000.0f, width / height,
 * fov), Matrix::lookAt(from, to, up).invert(), P.m[0] negated when flip_x == 1, then Camera::init /
 * updateView), so the records of a loaded scene's own pose and size are rtg_scene_desc.camera and
 * .projection byte for byte. They are what rtg_set_camera (include/rtg.h) takes. RTG_ERR_ARG, with the
 * outputs left as they were: a null pointer, a non-finite from, to, up or fov, from == to (or a distance
 * that overflows), up parallel to from - to (up x normalize(from - to) zero or overflowed), width or
 * height <= 0. */
int  rth_camera_look_at(const float from[3], const float to[3], const float up[3], float fov_degrees, int32_t width,
                        int32_t height, int32_t flip_x, rtg_camera* cam, rtg_camera_proj* proj);
/* What the loaded scene.json said (defaults: fov 45, flipX 0, vectors 0); any output may be NULL. */
int  rth_scene_camera_pose(const rth_scene* s, float from[3], float to[3], float up[3], float* fov, int32_t* flip_x);

/* Film::save: divide the accumulated sum by spp and write RLE RGBE (.hdr). */
int  rth_save_hdr(const char* path, int32_t width, int32_t height, const float* rgb_sum, uint32_t spp);
/* Film::tonemap (Imaging.h:233-242) for every pixel: (sum*exposure/(float)spp) clamped at 0,
 * powf(.., 1/2.2f)*255 clamped at 255, truncated to a byte. rgb8 receives width*height*3 bytes. */
int  rth_tonemap(int32_t width, int32_t height, const float* rgb_sum, uint32_t spp, float exposure, uint8_t* rgb8);
/* RayTracer::savePNG (Renderer.h:895-898): tonemapped film written as an 8-bit RGB PNG. */
int  rth_save_png(const char* path, int32_t width, int32_t height, const float* rgb_sum, uint32_t spp);
/* Plain RGBE writer for an already-normalised float RGB image. */
int  rth_write_hdr(const char* path, int32_t width, int32_t height, const float* rgb);
/* Radiance .hdr reader (stbi_loadf semantics, 3 channels). Caller frees with rth_free. */
int  rth_read_hdr(const char* path, int32_t* width, int32_t* height, float** rgb);
/* 8-bit PNG reader (stbi_load semantics). Caller frees with rth_free. */
int  rth_read_png(const char* path, int32_t* width, int32_t* height, int32_t* channels, uint8_t** data);
/* 8-bit texture decode as Texture::load's stbi_load sees it (Imaging.h:50): PNG or JPEG (baseline
 * and progressive) chosen by content; channels = 1 or 3 for JPEG. Free with rth_free. */
int  rth_read_ldr(const char* path, int32_t* width, int32_t* height, int32_t* channels, uint8_t** data);
void rth_free(void* p);

/* C3 synthetic scene: n_tris random triangles, splitmix64 stream from seed,
 * written as .gem + scene.json + albedo .png + constant env.hdr so rth_load_scene loads it. */
int  rth_write_synthetic(const char* dir, uint32_t n_tris, uint64_t seed, int32_t width, int32_t height);
/* The same scene recipe around caller-given triangles (positions: 9 floats per triangle, face normals). */
int  rth_write_mesh_scene(const char* dir, const float* positions, uint32_t n_tris, int32_t width, int32_t height);

#ifdef __cplusplus
}
#endif
#endif /* RTH_H */
