"""Python mirror of RTBase's host-facing API on top of the native libraries.

  loadScene(name, ...)          -> Scene         RTBase/SceneLoader.h:237-291 (librth)
  RayTracer(scene, device)      .init/.render/.getSPP/.clear/.saveHDR   RTBase/Renderer.h:45-898
  Scene.triangles/.lights       post-BVH-build arrays (numpy views of the flattened Scene)

RayTracer.render() is the drop-in for RayTracer::render(): it adds one sample per pixel through
the HIP wavefront path tracer (librtg). There is no CPU fallback; without a GPU, RayTracer raises.
"""
import ctypes as C
import os

import numpy as np

from . import _native as N


class NativeError(RuntimeError):
    pass


def _check(rc, lib_err):
    if rc != 0:
        raise NativeError("%s (code %d)" % (lib_err().decode(errors="replace"), rc))


class Scene:
    """The flattened reference Scene produced by the host front-end (rth_load_scene)."""

    def __init__(self, handle):
        self._h = handle
        self.desc_ptr = N.rth().rth_scene_desc(handle)
        self.desc = self.desc_ptr.contents
        info = N.rth_scene_info()
        _check(N.rth().rth_scene_get_info(handle, C.byref(info)), N.rth().rth_last_error)
        self.info = info
        self.width, self.height = info.width, info.height

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            N.rth().rth_free_scene(h)

    # numpy views (no copy) of the flattened arrays; each view keeps this Scene alive
    def _view(self, p, n, dtype):
        if n == 0:
            return np.zeros(0, dtype)
        ctype = p._type_
        buf = (ctype * n).from_address(C.addressof(p.contents))
        buf._owner = self
        return np.frombuffer(buf, dtype=np.dtype(ctype)).view(dtype)

    @property
    def positions(self):
        return self._view(self.desc.positions, self.desc.n_tris * 9, np.float32).reshape(-1, 3, 3)

    @property
    def normals(self):
        return self._view(self.desc.normals, self.desc.n_tris * 9, np.float32).reshape(-1, 3, 3)

    @property
    def uvs(self):
        return self._view(self.desc.uvs, self.desc.n_tris * 6, np.float32).reshape(-1, 3, 2)

    @property
    def material_index(self):
        return self._view(self.desc.material, self.desc.n_tris, np.uint32)

    @property
    def node_bounds(self):
        return self._view(self.desc.node_bounds, self.desc.n_nodes * 6, np.float32).reshape(-1, 6)

    @property
    def node_links(self):
        return self._view(self.desc.node_links, self.desc.n_nodes * 4, np.int32).reshape(-1, 4)

    @property
    def lights(self):
        return self._view(self.desc.lights, self.desc.n_lights, np.int32)

    @property
    def materials(self):
        return [self.desc.materials[i] for i in range(self.desc.n_materials)]

    @property
    def material_params(self):
        """What the reference's loader hands the BSDF constructors, one rtg_material_params per entry of
        `materials` in that order (rth_scene_material_params): model tag, alpha = 1.62142f *
        sqrtf(roughness), sigma, eta, k, int_ior, ext_ior. RayTracer.set_material_model passes them on."""
        n = C.c_uint32()
        p = N.rth().rth_scene_material_params(self._h, C.byref(n))
        return [N.rtg_material_params.from_buffer_copy(p[i]) for i in range(n.value)]  # (copies: they outlive the scene)

    @property
    def material_params_transmissive(self):
        """material_params with the loader's rough dielectrics tagged RTG_MODEL_ROUGH_DIELECTRIC
        (rth_scene_material_params_transmissive): what set_material_model("physical", transmission=True)
        passes on. Every other record equals material_params' field for field."""
        n = C.c_uint32()
        p = N.rth().rth_scene_material_params_transmissive(self._h, C.byref(n))
        return [N.rtg_material_params.from_buffer_copy(p[i]) for i in range(n.value)]

    def texture(self, i):
        t = self.desc.textures[i]
        return self._view(t.texels, t.width * t.height * 3, np.float32).reshape(t.height, t.width, 3)

    @property
    def camera(self):
        c = self.desc.camera
        return {"inv_proj": np.array(c.inv_proj[:], np.float32).reshape(4, 4),
                "camera": np.array(c.camera[:], np.float32).reshape(4, 4),
                "origin": np.array(c.origin[:], np.float32), "width": c.width, "height": c.height}

    @property
    def camera_pose(self):
        """What scene.json said: {"from_", "to", "up" (3 floats each), "fov" (degrees), "flip_x"}
        (rth_scene_camera_pose). look_at(width=w, height=h, **pose) rebuilds desc.camera / desc.projection."""
        f, t, u = (np.zeros(3, np.float32) for _ in range(3))
        fov, flip = C.c_float(), C.c_int32()
        _check(N.rth().rth_scene_camera_pose(self._h, N.ptr(f, C.c_float), N.ptr(t, C.c_float), N.ptr(u, C.c_float),
                                             C.byref(fov), C.byref(flip)), N.rth().rth_last_error)
        return {"from_": f, "to": t, "up": u, "fov": fov.value, "flip_x": flip.value}

    def permutation(self):
        out = np.zeros(self.desc.n_tris, np.uint32)
        _check(N.rth().rth_scene_permutation(self._h, N.ptr(out, C.c_uint32)), N.rth().rth_last_error)
        return out


def loadScene(scene_dir, width=0, height=0, skip_missing=False, envmap=None, bvh_threads=0):
    """RTBase loadScene(sceneName) with optional film-size / env overrides (applied before P)."""
    opts = N.rth_load_options(int(width), int(height), 1 if skip_missing else 0, int(bvh_threads),
                              envmap.encode() if envmap else None)
    h = C.c_void_p()
    _check(N.rth().rth_load_scene(os.fsencode(scene_dir), C.byref(opts), C.byref(h)), N.rth().rth_last_error)
    return Scene(h)


def look_at(from_, to, up, fov, width, height, flip_x=0):
    """The camera records of a pose, (rtg_camera, rtg_camera_proj), built by the loader's own code
    (rth_camera_look_at): what RayTracer.set_camera takes. Non-finite input, from_ == to, up parallel to
    the view or a non-positive size raises NativeError."""
    v = [np.ascontiguousarray(a, np.float32).reshape(-1) for a in (from_, to, up)]
    if any(len(a) != 3 for a in v):
        raise ValueError("look_at: from_, to and up take three floats each")
    cam, proj = N.rtg_camera(), N.rtg_camera_proj()
    _check(N.rth().rth_camera_look_at(N.ptr(v[0], C.c_float), N.ptr(v[1], C.c_float), N.ptr(v[2], C.c_float),
                                      float(fov), int(width), int(height), int(flip_x), C.byref(cam), C.byref(proj)),
           N.rth().rth_last_error)
    return cam, proj


def _temporal_params(max_history, plane_tolerance, normal_cos):
    return N.rtg_temporal_params(float(max_history), float(plane_tolerance), float(normal_cos))


def temporal_check(max_history=64.0, plane_tolerance=0.01, normal_cos=0.9):
    """rtg_temporal_check: the argument check of RayTracer.temporal alone (no device needed)."""
    p = _temporal_params(max_history, plane_tolerance, normal_cos)
    _check(N.rtg().rtg_temporal_check(C.byref(p)), N.rtg().rtg_last_error)


def temporal_defaults():
    p = N.rtg_temporal_params()
    _check(N.rtg().rtg_temporal_defaults(C.byref(p)), N.rtg().rtg_last_error)
    return {"max_history": p.max_history, "plane_tolerance": p.plane_tolerance, "normal_cos": p.normal_cos}


def _svgf_params(max_history, plane_tolerance, normal_cos, iterations, normal_squarings, sigma_luminance,
                 sigma_albedo, min_history, variance_floor):
    return N.rtg_svgf_params(_temporal_params(max_history, plane_tolerance, normal_cos), int(iterations),
                             int(normal_squarings), float(sigma_luminance), float(sigma_albedo), float(min_history),
                             float(variance_floor))


def svgf_check(max_history=64.0, plane_tolerance=0.01, normal_cos=0.9, iterations=5, normal_squarings=5,
               sigma_luminance=4.0, sigma_albedo=0.1, min_history=4.0, variance_floor=1e-8):
    """rtg_svgf_check: the argument check of RayTracer.svgf alone (no device needed)."""
    p = _svgf_params(max_history, plane_tolerance, normal_cos, iterations, normal_squarings, sigma_luminance,
                     sigma_albedo, min_history, variance_floor)
    _check(N.rtg().rtg_svgf_check(C.byref(p)), N.rtg().rtg_last_error)


def svgf_defaults():
    p = N.rtg_svgf_params()
    _check(N.rtg().rtg_svgf_defaults(C.byref(p)), N.rtg().rtg_last_error)
    return {"max_history": p.temporal.max_history, "plane_tolerance": p.temporal.plane_tolerance,
            "normal_cos": p.temporal.normal_cos, "iterations": p.iterations, "normal_squarings": p.normal_squarings,
            "sigma_luminance": p.sigma_luminance, "sigma_albedo": p.sigma_albedo, "min_history": p.min_history,
            "variance_floor": p.variance_floor}


def svgf_illum_check(albedo_floor=1e-3, **svgf):
    """rtg_svgf_illum_check: the argument check of RayTracer.svgf(illumination=True) alone (no device needed);
    the other keywords are svgf_check's."""
    d = svgf_defaults()
    d.update(svgf)
    p = N.rtg_svgf_illum_params(_svgf_params(**d), float(albedo_floor))
    _check(N.rtg().rtg_svgf_illum_check(C.byref(p)), N.rtg().rtg_last_error)


def svgf_illum_defaults():
    p = N.rtg_svgf_illum_params()
    _check(N.rtg().rtg_svgf_illum_defaults(C.byref(p)), N.rtg().rtg_last_error)
    s = p.svgf
    return {"max_history": s.temporal.max_history, "plane_tolerance": s.temporal.plane_tolerance,
            "normal_cos": s.temporal.normal_cos, "iterations": s.iterations, "normal_squarings": s.normal_squarings,
            "sigma_luminance": s.sigma_luminance, "sigma_albedo": s.sigma_albedo, "min_history": s.min_history,
            "variance_floor": s.variance_floor, "albedo_floor": p.albedo_floor}


def write_synthetic_scene(out_dir, n_tris=1_000_000, seed=20251015, width=1024, height=1024):
    """C3 synthetic scene as .gem + scene.json + albedo.png + env.hdr."""
    os.makedirs(out_dir, exist_ok=True)
    _check(N.rth().rth_write_synthetic(os.fsencode(out_dir), n_tris, seed, width, height), N.rth().rth_last_error)
    return out_dir


def write_mesh_scene(out_dir, positions, width=256, height=256):
    """The C3 scene recipe (diffuse albedo, constant env light, fixed camera) around caller-given
    triangles: positions (n, 3, 3) float32."""
    p = np.ascontiguousarray(positions, np.float32).reshape(-1, 9)
    os.makedirs(out_dir, exist_ok=True)
    _check(N.rth().rth_write_mesh_scene(os.fsencode(out_dir), N.ptr(p, C.c_float), len(p), width, height),
           N.rth().rth_last_error)
    return out_dir


def save_hdr(path, film_sum, spp):
    """Film::save: film / SPP -> RLE RGBE (stbi_write_hdr format)."""
    f = np.ascontiguousarray(film_sum, np.float32)
    h, w = f.shape[0], f.shape[1]
    _check(N.rth().rth_save_hdr(os.fsencode(path), w, h, N.ptr(f, C.c_float), spp), N.rth().rth_last_error)


def tonemap(film_sum, spp, exposure=1.0):
    """Film::tonemap (Imaging.h:233-242) of every pixel -> uint8 RGB (H, W, 3)."""
    f = np.ascontiguousarray(film_sum, np.float32)
    h, w = f.shape[0], f.shape[1]
    out = np.zeros((h, w, 3), np.uint8)
    _check(N.rth().rth_tonemap(w, h, N.ptr(f, C.c_float), spp, exposure, N.ptr(out, C.c_uint8)),
           N.rth().rth_last_error)
    return out


def save_png(path, film_sum, spp):
    """RayTracer::savePNG (Renderer.h:895-898): tonemapped film as an 8-bit RGB PNG."""
    f = np.ascontiguousarray(film_sum, np.float32)
    h, w = f.shape[0], f.shape[1]
    _check(N.rth().rth_save_png(os.fsencode(path), w, h, N.ptr(f, C.c_float), spp), N.rth().rth_last_error)


def read_hdr(path):
    w, h = C.c_int32(), C.c_int32()
    p = N.f32p()
    _check(N.rth().rth_read_hdr(os.fsencode(path), C.byref(w), C.byref(h), C.byref(p)), N.rth().rth_last_error)
    try:
        return np.ctypeslib.as_array(p, shape=(h.value, w.value, 3)).copy()
    finally:
        N.rth().rth_free(C.cast(p, C.c_void_p))


def _denoise_params(iterations, normal_squarings, sigma_colour, sigma_albedo):
    return N.rtg_denoise_params(int(iterations), int(normal_squarings), float(sigma_colour), float(sigma_albedo))


def denoise_images(colour, albedo, normal, device=0, iterations=5, normal_squarings=5, sigma_colour=1.0,
                   sigma_albedo=0.1):
    """The denoiser's filter alone (rtg_denoise_images) on caller-given (H, W, 3) float32 images: the
    edge-avoiding a-trous wavelet filter guided by albedo and normals (include/rtg.h). Returns (H, W, 3)."""
    c, a, n = (np.ascontiguousarray(v, np.float32) for v in (colour, albedo, normal))
    if c.ndim != 3 or c.shape[2] != 3 or a.shape != c.shape or n.shape != c.shape:
        raise ValueError("denoise_images: colour, albedo and normal must share one (H, W, 3) shape")
    out = np.zeros(c.shape, np.float32)
    p = _denoise_params(iterations, normal_squarings, sigma_colour, sigma_albedo)
    lib = N.rtg()
    _check(lib.rtg_denoise_images(device, c.shape[1], c.shape[0], N.ptr(c, C.c_float), N.ptr(a, C.c_float),
                                  N.ptr(n, C.c_float), C.byref(p), N.ptr(out, C.c_float)), lib.rtg_last_error)
    return out


def probe_texture(texels, coords, env=False, uniform=False):
    """The shading kernel's texture arithmetic alone (rtg_probe_texture, test surface) on a caller-given
    (H, W, 3) float32 texture, on the current device. env=False: Texture::sample at coords (n, 2) = (tu,
    tv); env=True: EnvironmentMap::evaluate at coords (n, 3), the direction. uniform=True takes the
    kernels' short-cut for a texture whose texels all have the same bits. Returns (n, 3) float32."""
    t = np.ascontiguousarray(texels, np.float32)
    if t.ndim != 3 or t.shape[2] != 3:
        raise ValueError("probe_texture: texels must be (H, W, 3)")
    c = np.ascontiguousarray(coords, np.float32).reshape(-1, 3 if env else 2)
    out = np.zeros((len(c), 3), np.float32)
    mode = (N.RTG_PROBE_TEX_ENV if env else N.RTG_PROBE_TEX_SAMPLE) | (N.RTG_PROBE_TEX_UNIFORM if uniform else 0)
    lib = N.rtg()
    _check(lib.rtg_probe_texture(mode, N.ptr(t, C.c_float), t.shape[1], t.shape[0], N.ptr(c, C.c_float), len(c),
                                 N.ptr(out, C.c_float)), lib.rtg_last_error)
    return out


FILTERS = {"none": N.RTG_FILTER_NONE, "box": N.RTG_FILTER_BOX, "tent": N.RTG_FILTER_TENT}
FILTER_DEFAULT_RADIUS = {N.RTG_FILTER_NONE: 0.5, N.RTG_FILTER_BOX: 0.5, N.RTG_FILTER_TENT: 1.0}


def _camera_sampling(filter, filter_radius, lens_radius, focal_distance):
    """The rtg_camera_sampling of set_camera_sampling's arguments (filter: a name of FILTERS or an
    RTG_FILTER_* value; filter_radius None: the filter's default). Range errors are the library's."""
    if isinstance(filter, str):
        if filter not in FILTERS:
            raise ValueError("unknown pixel filter %r (one of %s)" % (filter, ", ".join(FILTERS)))
        filter = FILTERS[filter]
    filter = int(filter)
    if filter_radius is None:
        filter_radius = FILTER_DEFAULT_RADIUS.get(filter, 0.5)
    return N.rtg_camera_sampling(filter, float(filter_radius), float(lens_radius), float(focal_distance))


ENV_SAMPLING = {"uniform": N.RTG_ENV_UNIFORM, "luminance": N.RTG_ENV_LUMINANCE}


def _env_mode(mode):
    """The RTG_ENV_* value of set_env_sampling's argument (a name of ENV_SAMPLING or a value; an
    unknown value is the library's error)."""
    if isinstance(mode, str):
        if mode not in ENV_SAMPLING:
            raise ValueError("unknown environment sampling %r (one of %s)" % (mode, ", ".join(ENV_SAMPLING)))
        return ENV_SAMPLING[mode]
    return int(mode)


LIGHT_SAMPLING = {"uniform": N.RTG_LIGHTS_UNIFORM, "power": N.RTG_LIGHTS_POWER}


def _light_sampling(mode, uniform_share):
    """The rtg_light_sampling of set_light_sampling's arguments (a name of LIGHT_SAMPLING or a value; an
    unknown value or a share outside [0, 1] is the library's error)."""
    if isinstance(mode, str):
        if mode not in LIGHT_SAMPLING:
            raise ValueError("unknown light sampling %r (one of %s)" % (mode, ", ".join(LIGHT_SAMPLING)))
        mode = LIGHT_SAMPLING[mode]
    return N.rtg_light_sampling(int(mode), float(uniform_share))


MATERIAL_MODELS = {"reference": N.RTG_MATERIALS_REFERENCE, "physical": N.RTG_MATERIALS_PHYSICAL}
MODEL_TAGS = {"conductor": N.RTG_MODEL_CONDUCTOR, "plastic": N.RTG_MODEL_PLASTIC, "orennayar": N.RTG_MODEL_ORENNAYAR,
              "rough_dielectric": N.RTG_MODEL_ROUGH_DIELECTRIC}


def _material_model(mode):
    """The RTG_MATERIALS_* value of set_material_model's argument (a name of MATERIAL_MODELS or a value;
    an unknown value is the library's error)."""
    if isinstance(mode, str):
        if mode not in MATERIAL_MODELS:
            raise ValueError("unknown material model %r (one of %s)" % (mode, ", ".join(MATERIAL_MODELS)))
        return MATERIAL_MODELS[mode]
    return int(mode)


PATH_MIS = {"off": N.RTG_PATH_MIS_OFF, "power": N.RTG_PATH_MIS_POWER}


def _path_mis(mode):
    """The RTG_PATH_MIS_* value of set_path_mis's argument (a name of PATH_MIS or a value; an unknown
    value is the library's error)."""
    if isinstance(mode, str):
        if mode not in PATH_MIS:
            raise ValueError("unknown path MIS mode %r (one of %s)" % (mode, ", ".join(PATH_MIS)))
        return PATH_MIS[mode]
    return int(mode)


def path_mis_check(mode):
    """rtg_set_path_mis's argument check alone (rtg_path_mis_check; no GPU): raises NativeError for an
    unknown mode."""
    lib = N.rtg()
    _check(lib.rtg_path_mis_check(_path_mis(mode)), lib.rtg_last_error)


SAMPLERS = {"pcg": N.RTG_SAMPLER_PCG, "sobol": N.RTG_SAMPLER_SOBOL}


def _sampler(name):
    """The RTG_SAMPLER_* value of set_sampler's argument (a name of SAMPLERS or a value; an unknown value
    is the library's error)."""
    if isinstance(name, str):
        if name not in SAMPLERS:
            raise ValueError("unknown sampler %r (one of %s)" % (name, ", ".join(SAMPLERS)))
        return SAMPLERS[name]
    return int(name)


def sampler_check(name):
    """rtg_set_sampler's argument check alone (rtg_sampler_check; no GPU): raises NativeError for an
    unknown value."""
    lib = N.rtg()
    _check(lib.rtg_sampler_check(_sampler(name)), lib.rtg_last_error)


def mis_weight_probe(p, q):
    """The path-tracer MIS kernels' own weight function (rtg_probe_mis_weight, test surface) on the
    current device: mis_w(p[i], q[i]) for p, q (n,) float32."""
    p, q = (np.ascontiguousarray(v, np.float32).reshape(-1) for v in (p, q))
    if len(p) != len(q):
        raise ValueError("mis_weight_probe: p and q must have one length")
    w = np.zeros(len(p), np.float32)
    lib = N.rtg()
    _check(lib.rtg_probe_mis_weight(N.ptr(p, C.c_float), N.ptr(q, C.c_float), len(p), N.ptr(w, C.c_float)),
           lib.rtg_last_error)
    return w


def _material_params_array(params):
    """A ctypes array of rtg_material_params from a sequence of them."""
    params = list(params)
    return (N.rtg_material_params * max(len(params), 1))(*params), len(params)


def _material_params_choice(rt, m, transmission, setter, handle):
    """set_material_model's parameter hand-over for a RayTracer or a RayTracerGroup: the scene's records
    (the transmissive set when asked for) go to the library before the first "physical" setting and again
    when the choice changes."""
    want = bool(transmission)
    if want and m != N.RTG_MATERIALS_PHYSICAL:
        raise ValueError("transmission=True needs the \"physical\" material model")
    if m != N.RTG_MATERIALS_PHYSICAL:
        return
    if getattr(rt, "_material_params_set", False) and getattr(rt, "_material_params_trans", False) == want:
        return
    arr, n = _material_params_array(rt.scene.material_params_transmissive if want else rt.scene.material_params)
    _check(setter(handle, arr, n), rt._lib.rtg_last_error)
    rt._material_params_set = True
    rt._material_params_trans = want


def transmission_probe(wo, draws, query, alpha=0.5, int_ior=1.5, ext_ior=1.0, albedo=(1.0, 1.0, 1.0),
                       normal=(0.0, 0.0, 1.0)):
    """The rough dielectric kernels' own sample / evaluate / PDF (rtg_probe_transmission, test surface) on
    the current device, as material_probe: wo (n, 3), draws (n, 3) and query (n, 3) per case, world space,
    anywhere on the sphere, with one parameter set, albedo and shading normal for all. Returns
    material_probe's dict."""
    wo, dr, qi = (np.ascontiguousarray(v, np.float32).reshape(-1, 3) for v in (wo, draws, query))
    if not len(wo) == len(dr) == len(qi):
        raise ValueError("transmission_probe: wo, draws and query must have one length")
    c = np.zeros((len(wo), 28), np.float32)
    c[:, 0:5] = (N.RTG_MODEL_ROUGH_DIELECTRIC, alpha, 0.0, int_ior, ext_ior)
    c[:, 11:14], c[:, 14:17] = albedo, normal
    c[:, 17:20], c[:, 20:23], c[:, 23:26] = wo, dr, qi
    out = np.zeros((len(wo), 16), np.float32)
    lib = N.rtg()
    _check(lib.rtg_probe_transmission(N.ptr(c, C.c_float), len(c), N.ptr(out, C.c_float)), lib.rtg_last_error)
    return {"wi": out[:, 0:3].copy(), "colour": out[:, 3:6].copy(), "pdf": out[:, 6].copy(),
            "draws": out[:, 7].astype(np.int32), "delta": out[:, 8] != 0, "evaluate": out[:, 9:12].copy(),
            "PDF": out[:, 12].copy()}


def material_params_check(params, n_materials):
    """rtg_set_material_params' argument check alone (rtg_material_params_check; no GPU): raises
    NativeError for a wrong count, an unknown tag or a negative or non-finite parameter."""
    arr, n = _material_params_array(params)
    lib = N.rtg()
    _check(lib.rtg_material_params_check(arr, n, n_materials), lib.rtg_last_error)


def material_probe(model, wo, draws, query, alpha=0.0, sigma=0.0, int_ior=1.33, ext_ior=1.0, eta=(0.0, 0.0, 0.0),
                   k=(0.0, 0.0, 0.0), albedo=(1.0, 1.0, 1.0), normal=(0.0, 0.0, 1.0)):
    """The physical material kernels' own sample / evaluate / PDF (rtg_probe_material, test surface) on
    the current device. model: a name of MODEL_TAGS or a tag; wo (n, 3), draws (n, 3) and query (n, 3)
    per case, world space, with one parameter set, albedo and shading normal for all. Returns a dict:
    "wi" (n, 3), "colour" (n, 3), "pdf", "draws", "delta" (n,), "evaluate" (n, 3), "PDF" (n,)."""
    tag = MODEL_TAGS[model] if isinstance(model, str) else int(model)
    wo, dr, qi = (np.ascontiguousarray(v, np.float32).reshape(-1, 3) for v in (wo, draws, query))
    if not len(wo) == len(dr) == len(qi):
        raise ValueError("material_probe: wo, draws and query must have one length")
    c = np.zeros((len(wo), 28), np.float32)
    c[:, 0:5] = (tag, alpha, sigma, int_ior, ext_ior)
    c[:, 5:8], c[:, 8:11], c[:, 11:14], c[:, 14:17] = eta, k, albedo, normal
    c[:, 17:20], c[:, 20:23], c[:, 23:26] = wo, dr, qi
    out = np.zeros((len(wo), 16), np.float32)
    lib = N.rtg()
    _check(lib.rtg_probe_material(N.ptr(c, C.c_float), len(c), N.ptr(out, C.c_float)), lib.rtg_last_error)
    return {"wi": out[:, 0:3].copy(), "colour": out[:, 3:6].copy(), "pdf": out[:, 6].copy(),
            "draws": out[:, 7].astype(np.int32), "delta": out[:, 8] != 0, "evaluate": out[:, 9:12].copy(),
            "PDF": out[:, 12].copy()}


class RayTracer:
    """RayTracer (Renderer.h:31-899) backed by librtg on one GPU."""

    MAX_DEPTH = 4  # Renderer.h:20

    INTEGRATORS = {"path": N.RTG_INTEGRATOR_PATH, "direct": N.RTG_INTEGRATOR_DIRECT,
                   "albedo": N.RTG_INTEGRATOR_ALBEDO, "normals": N.RTG_INTEGRATOR_NORMALS,
                   "direct_mis": N.RTG_INTEGRATOR_DIRECT_MIS}

    def __init__(self, scene, device=0, max_depth=MAX_DEPTH, seed=1234, cull=True, max_paths=0, wide=True,
                 integrator="path"):
        self.scene = scene
        self.seed = seed
        self._lib = N.rtg()
        h = C.c_void_p()
        _check(self._lib.rtg_create(device, scene.desc_ptr, C.byref(h)), self._lib.rtg_last_error)
        self._h = h
        self.width, self.height = scene.width, scene.height
        self.max_depth = max_depth
        self.flags = (N.RTG_OPT_CULL if cull else 0) | (0 if wide else N.RTG_OPT_BVH2)
        self.set_options(max_depth=max_depth, flags=self.flags, max_paths=max_paths)
        self.set_integrator(integrator)

    def set_integrator(self, integrator):
        """Per-pixel estimator: "path" (pathTrace, default), "direct", "albedo", "normals"
        (RayTracer::direct / albedo / viewNormals, Renderer.h:393-407, 558-582), "direct_mis"
        (direct() with computeDirectMIS, Renderer.h:474-557)."""
        mode = self.INTEGRATORS[integrator] if isinstance(integrator, str) else int(integrator)
        _check(self._lib.rtg_set_integrator(self._h, mode), self._lib.rtg_last_error)
        self.integrator = integrator

    def set_camera(self, camera, projection):
        """Replace the camera of the live tracer (rtg_set_camera): an rtg_camera and an rtg_camera_proj,
        e.g. from look_at(). Frames queued earlier keep the camera they were queued under; the film and
        SPP are left alone (clear() them, as Main.cpp does after a move); the denoiser's guides are
        rendered again by the next denoise(). The film size cannot change."""
        _check(self._lib.rtg_set_camera(self._h, C.byref(camera), C.byref(projection)), self._lib.rtg_last_error)

    def look_at(self, from_, to, up, fov=None):
        """set_camera(*look_at(...)) at this tracer's film size, with the scene's flipX and, for fov None,
        the scene's fov."""
        pose = self.scene.camera_pose
        self.set_camera(*look_at(from_, to, up, pose["fov"] if fov is None else fov, self.width, self.height,
                                 pose["flip_x"]))

    def camera(self):
        """(rtg_camera, rtg_camera_proj): the records in use (rtg_get_camera)."""
        cam, proj = N.rtg_camera(), N.rtg_camera_proj()
        _check(self._lib.rtg_get_camera(self._h, C.byref(cam), C.byref(proj)), self._lib.rtg_last_error)
        return cam, proj

    def geometry_guide(self):
        """(pos_t, normal_id), (H, W, 4) float32 each: per pixel the first hit of the pinhole ray through
        its centre, {X.xyz, t} and {unit geometric normal, triangle id as bits}; a miss is {0, 0, 0,
        FLT_MAX} {0, 0, 0, -1} (rtg_geometry_guide). normal_id[..., 3].view(np.int32) gives the ids."""
        a = np.zeros((self.height, self.width, 4), np.float32)
        b = np.zeros((self.height, self.width, 4), np.float32)
        _check(self._lib.rtg_geometry_guide(self._h, N.ptr(a, C.c_float), N.ptr(b, C.c_float)),
               self._lib.rtg_last_error)
        return a, b

    def temporal(self, max_history=64.0, plane_tolerance=0.01, normal_cos=0.9):
        """Temporal accumulation by reprojection (rtg_temporal_accumulate): film / SPP blended into a
        per-pixel history that follows set_camera() through the scene's geometry. The loop is: move,
        clear(), render(), temporal(). Returns the (H, W, 3) float32 image; the film, SPP and the settings
        stay as they were. Waits for queued frames first."""
        out = np.zeros((self.height, self.width, 3), np.float32)
        p = _temporal_params(max_history, plane_tolerance, normal_cos)
        _check(self._lib.rtg_temporal_accumulate(self._h, C.byref(p), N.ptr(out, C.c_float)),
               self._lib.rtg_last_error)
        return out

    def temporal_history(self):
        """The history, (H, W, 4) float32: rgb and the effective sample count len."""
        out = np.zeros((self.height, self.width, 4), np.float32)
        _check(self._lib.rtg_temporal_history(self._h, N.ptr(out, C.c_float)), self._lib.rtg_last_error)
        return out

    def temporal_reset(self):
        """Drop the history, its camera and the cached guides (rtg_temporal_reset)."""
        _check(self._lib.rtg_temporal_reset(self._h), self._lib.rtg_last_error)

    def copy_temporal_to(self, device_ptr):
        """The last temporal() result, (H, W, 3) float32, copied to device memory on this GPU."""
        _check(self._lib.rtg_temporal_copy_device(self._h, C.c_void_p(device_ptr)), self._lib.rtg_last_error)

    def temporal_ms(self):
        """(guide_ms, accumulate_ms): device time of the last call's guide pass (0 when none ran) and of
        its k_temporal launch."""
        g, a = C.c_double(), C.c_double()
        _check(self._lib.rtg_temporal_ms(self._h, C.byref(g), C.byref(a)), self._lib.rtg_last_error)
        return g.value, a.value

    def svgf(self, max_history=64.0, plane_tolerance=0.01, normal_cos=0.9, iterations=5, normal_squarings=5,
             sigma_luminance=4.0, sigma_albedo=0.1, min_history=4.0, variance_floor=1e-8, illumination=False,
             albedo_floor=1e-3):
        """Variance-guided filtering of the temporal history (rtg_svgf_accumulate): temporal()'s step on the
        same history, a moments history next to it, a per-pixel variance (spatial below min_history) and
        `iterations` a-trous levels whose luminance term that variance scales, all on the device. The loop is:
        move, clear(), render(), svgf(). Returns the (H, W, 3) float32 image; the film, SPP and the settings
        stay as they were. Waits for queued frames first.
        illumination=True (rtg_svgf_illum_accumulate): the same chain on the film over the first hit's albedo
        (channels at or below albedo_floor are not divided), multiplied back at the end, with directly seen
        emitters in a class of their own, over a history of the mode's own: temporal_history() and the default
        mode's state are not touched by it, nor its state by them."""
        out = np.zeros((self.height, self.width, 3), np.float32)
        p = _svgf_params(max_history, plane_tolerance, normal_cos, iterations, normal_squarings, sigma_luminance,
                         sigma_albedo, min_history, variance_floor)
        if illumination:
            q = N.rtg_svgf_illum_params(p, float(albedo_floor))
            _check(self._lib.rtg_svgf_illum_accumulate(self._h, C.byref(q), N.ptr(out, C.c_float)),
                   self._lib.rtg_last_error)
            return out
        _check(self._lib.rtg_svgf_accumulate(self._h, C.byref(p), N.ptr(out, C.c_float)), self._lib.rtg_last_error)
        return out

    def svgf_variance(self, illumination=False):
        """The variance the last svgf() fed to its first level, (H, W) float32 (illumination: of that mode)."""
        out = np.zeros((self.height, self.width), np.float32)
        f = self._lib.rtg_svgf_illum_variance if illumination else self._lib.rtg_svgf_variance
        _check(f(self._h, N.ptr(out, C.c_float)), self._lib.rtg_last_error)
        return out

    def svgf_moments(self, illumination=False):
        """The moments history, (H, W, 2) float32: the first two moments of the luminance (illumination: of that
        mode's demodulated film)."""
        out = np.zeros((self.height, self.width, 2), np.float32)
        f = self._lib.rtg_svgf_illum_moments if illumination else self._lib.rtg_svgf_moments
        _check(f(self._h, N.ptr(out, C.c_float)), self._lib.rtg_last_error)
        return out

    def copy_svgf_to(self, device_ptr, illumination=False):
        """The last svgf() result (illumination: of that mode), (H, W, 3) float32, copied to device memory on
        this GPU."""
        f = self._lib.rtg_svgf_illum_copy_device if illumination else self._lib.rtg_svgf_copy_device
        _check(f(self._h, C.c_void_p(device_ptr)), self._lib.rtg_last_error)

    def svgf_ms(self, illumination=False):
        """(guide_ms, accumulate_ms, variance_ms, filter_ms): device time of the last svgf()'s guide pass (0
        when none ran), temporal + moments kernel, variance kernel and filter levels together. illumination:
        that mode's last call, with (prepare_ms, unpack_ms) of its two own kernels appended."""
        v = [C.c_double() for _ in range(6 if illumination else 4)]
        f = self._lib.rtg_svgf_illum_ms if illumination else self._lib.rtg_svgf_ms
        _check(f(self._h, *[C.byref(x) for x in v]), self._lib.rtg_last_error)
        return tuple(x.value for x in v)

    def svgf_illum_history(self):
        """The illumination mode's history, (H, W, 4) float32: the demodulated rgb and len."""
        out = np.zeros((self.height, self.width, 4), np.float32)
        _check(self._lib.rtg_svgf_illum_history(self._h, N.ptr(out, C.c_float)), self._lib.rtg_last_error)
        return out

    def svgf_illum_guide(self):
        """(pos_t, normal_id) as geometry_guide() gives them, of the illumination history's camera and classed:
        a pixel whose first hit is an emitter carries the miss records."""
        a = np.zeros((self.height, self.width, 4), np.float32)
        b = np.zeros((self.height, self.width, 4), np.float32)
        _check(self._lib.rtg_svgf_illum_guide(self._h, N.ptr(a, C.c_float), N.ptr(b, C.c_float)),
               self._lib.rtg_last_error)
        return a, b

    def gbuffer(self):
        """The first-hit AOVs of the current camera from one traversal of its pixel-centre rays (rtg_gbuffer):
        "pos_t" and "normal_id", (H, W, 4) float32, are geometry_guide()'s two images; "albedo" and "normal",
        (H, W, 3) float32, are guides()'s. Depth is pos_t[..., 3] (FLT_MAX on a miss), the triangle id
        normal_id[..., 3].view(np.int32) (-1 on a miss). The call fills the caches those calls, temporal(),
        svgf() and denoise() read, so none of them traces a camera ray afterwards until set_camera(). The film,
        SPP and the settings stay as they were. Waits for queued frames first."""
        shape = (self.height, self.width)
        out = {"pos_t": np.zeros(shape + (4,), np.float32), "normal_id": np.zeros(shape + (4,), np.float32),
               "albedo": np.zeros(shape + (3,), np.float32), "normal": np.zeros(shape + (3,), np.float32)}
        ptrs = [N.ptr(out[k], C.c_float) for k in ("pos_t", "normal_id", "albedo", "normal")]
        _check(self._lib.rtg_gbuffer(self._h, *ptrs), self._lib.rtg_last_error)
        return out

    def gbuffer_ms(self):
        """Device time of the fused first-hit pass in the last gbuffer() or svgf(), in ms (0 when the caches
        served it)."""
        v = C.c_double()
        _check(self._lib.rtg_gbuffer_ms(self._h, C.byref(v)), self._lib.rtg_last_error)
        return v.value

    def set_camera_sampling(self, filter="none", filter_radius=None, lens_radius=0.0, focal_distance=1.0):
        """Anti-aliasing and depth of field (rtg_set_camera_sampling). filter "none" (default: every
        sample through the pixel centre, as renderTile), "box" or "tent": sample s of a pixel crosses
        the film at an offset drawn from the filter (radius in pixels; None: 0.5 for the box, 1 for
        the tent) and still counts for its own pixel only. lens_radius > 0: a thin lens focused at
        focal_distance along the view direction. Applies to render(), adaptiveRender() and every
        integrator; not to lightTracer(), instantRadiosity() or the denoiser's guides."""
        p = _camera_sampling(filter, filter_radius, lens_radius, focal_distance)
        _check(self._lib.rtg_set_camera_sampling(self._h, C.byref(p)), self._lib.rtg_last_error)

    def camera_sampling(self):
        """The current setting: {"filter": name, "filter_radius", "lens_radius", "focal_distance"}."""
        p = N.rtg_camera_sampling()
        _check(self._lib.rtg_get_camera_sampling(self._h, C.byref(p)), self._lib.rtg_last_error)
        names = {v: k for k, v in FILTERS.items()}
        return {"filter": names.get(p.filter, p.filter), "filter_radius": p.filter_radius,
                "lens_radius": p.lens_radius, "focal_distance": p.focal_distance}

    def camera_samples(self, pixels, samples, seed=None):
        """The camera rays the renderer generates for the given (pixel index y * W + x, sample index)
        pairs under the current setting (rtg_probe_camera_samples; seed None: this tracer's).
        Returns (rays (n, 8) = o.xyz, 0, d.xyz, 0 as trace_closest takes them, film_xy (n, 2))."""
        px = np.ascontiguousarray(pixels, np.uint32).reshape(-1)
        sm = np.ascontiguousarray(samples, np.uint32).reshape(-1)
        if len(px) != len(sm):
            raise ValueError("camera_samples: pixels and samples must have one length")
        rays = np.zeros((len(px), 8), np.float32)
        xy = np.zeros((len(px), 2), np.float32)
        _check(self._lib.rtg_probe_camera_samples(self._h, N.ptr(px, C.c_uint32), N.ptr(sm, C.c_uint32), len(px),
                                                  self.seed if seed is None else seed, N.ptr(rays, C.c_float),
                                                  N.ptr(xy, C.c_float)), self._lib.rtg_last_error)
        return rays, xy

    def set_env_sampling(self, mode="uniform"):
        """How NEE samples the environment light (rtg_set_env_sampling). "uniform" (default):
        EnvironmentMap::sample's uniform sphere, the reference's films bit for bit. "luminance":
        directions drawn in proportion to the map's filtered luminance times sin theta through an
        alias table (built on the first use, kept with the tracer): the same expectation with far
        less noise under a map whose light sits in a sun or a window; it draws four numbers per
        environment sample instead of two, so its films are not the uniform mode's. A scene without
        an environment light, or a black map, keeps sampling uniformly. Applies to render(),
        adaptiveRender() and the "path", "direct" and "direct_mis" integrators; not to lightTracer(),
        instantRadiosity() or the denoiser's guides."""
        _check(self._lib.rtg_set_env_sampling(self._h, _env_mode(mode)), self._lib.rtg_last_error)

    def env_sampling(self):
        """The current setting, "uniform" or "luminance"."""
        m = C.c_int()
        _check(self._lib.rtg_get_env_sampling(self._h, C.byref(m)), self._lib.rtg_last_error)
        return {v: k for k, v in ENV_SAMPLING.items()}.get(m.value, m.value)

    def env_table(self):
        """The active alias table (rtg_env_table): a dict of "prob" (H, W) float32, "alias" (H, W)
        uint32, "cellpdf_self" and "cellpdf_alias" (H, W) float32, "entries" (H * W, 4) uint32 (the
        words as the kernel loads them), "weights" (H, W) float64 (the cell weights it was built from)
        and "build_ms"; None when no table is active (uniform mode, no environment light, a black map)."""
        w, h, ms = C.c_uint32(), C.c_uint32(), C.c_double()
        _check(self._lib.rtg_env_table(self._h, C.byref(w), C.byref(h), None, C.byref(ms)), self._lib.rtg_last_error)
        if w.value == 0 or h.value == 0:
            return None
        e = np.zeros((w.value * h.value, 4), np.float32)
        _check(self._lib.rtg_env_table(self._h, C.byref(w), C.byref(h), N.ptr(e, C.c_float), None),
               self._lib.rtg_last_error)
        wt = np.zeros((h.value, w.value), np.float64)
        _check(self._lib.rtg_env_weights(self._h, N.ptr(wt, C.c_double)), self._lib.rtg_last_error)
        u = e.view(np.uint32)
        shape = (h.value, w.value)
        return {"prob": e[:, 0].reshape(shape).copy(), "alias": u[:, 1].reshape(shape).copy(),
                "cellpdf_self": e[:, 2].reshape(shape).copy(), "cellpdf_alias": e[:, 3].reshape(shape).copy(),
                "entries": u.copy(), "weights": wt, "build_ms": ms.value}

    def env_samples(self, r0, d):
        """The shading kernel's own environment sample (rtg_probe_env_samples) for scripted draws
        r0 (n,) uint32 and d (n, 3) = d1, d2, d3 against the active table: (wi (n, 3), pdf (n,)),
        pdf 0 where the sample is rejected."""
        r = np.ascontiguousarray(r0, np.uint32).reshape(-1)
        dd = np.ascontiguousarray(d, np.float32).reshape(-1, 3)
        if len(r) != len(dd):
            raise ValueError("env_samples: r0 and d must have one length")
        out = np.zeros((len(r), 4), np.float32)
        _check(self._lib.rtg_probe_env_samples(self._h, N.ptr(r, C.c_uint32), N.ptr(dd, C.c_float), len(r),
                                               N.ptr(out, C.c_float)), self._lib.rtg_last_error)
        return out[:, :3].copy(), out[:, 3].copy()

    def set_light_sampling(self, mode="uniform", uniform_share=0.125):
        """Which light an NEE sample goes to (rtg_set_light_sampling). "uniform" (default):
        Scene::sampleLight's pick, every entry of the light list (one per emissive triangle, plus the
        environment) equally often, the reference's films bit for bit. "power": light i with probability
        (1 - uniform_share) * w_i / sum(w) + uniform_share / n, w its luminance times area (the
        environment: its map's flux through the scene's bounding sphere over pi), through an alias
        table: the same expectation with less noise where a few lights carry most of the power; it
        draws two numbers per pick instead of one, so its films are not the uniform mode's. One light,
        or no power at all, keeps the uniform pick. Applies to render(), adaptiveRender() and the "path",
        "direct" and "direct_mis" integrators; not to lightTracer(), instantRadiosity(), the denoiser's
        guides, "albedo" or "normals"."""
        p = _light_sampling(mode, uniform_share)
        _check(self._lib.rtg_set_light_sampling(self._h, C.byref(p)), self._lib.rtg_last_error)

    def light_sampling(self):
        """The current setting: {"mode": "uniform" or "power", "uniform_share"}."""
        p = N.rtg_light_sampling()
        _check(self._lib.rtg_get_light_sampling(self._h, C.byref(p)), self._lib.rtg_last_error)
        return {"mode": {v: k for k, v in LIGHT_SAMPLING.items()}.get(p.mode, p.mode), "uniform_share": p.uniform_share}

    def light_table(self):
        """The active light-pick table (rtg_light_table): a dict of "prob" (n,) float32, "alias" (n,)
        uint32, "pmf_self" and "pmf_alias" (n,) float32, "entries" (n, 4) uint32 (the words as the kernel
        loads them), "weights" (n,) float64 and "build_ms"; None when no table is active (uniform mode,
        one light, no power)."""
        n, ms = C.c_uint32(), C.c_double()
        _check(self._lib.rtg_light_table(self._h, C.byref(n), None, C.byref(ms)), self._lib.rtg_last_error)
        if n.value == 0:
            return None
        e = np.zeros((n.value, 4), np.float32)
        _check(self._lib.rtg_light_table(self._h, C.byref(n), N.ptr(e, C.c_float), None), self._lib.rtg_last_error)
        wt = np.zeros(n.value, np.float64)
        _check(self._lib.rtg_light_weights(self._h, N.ptr(wt, C.c_double)), self._lib.rtg_last_error)
        u = e.view(np.uint32)
        return {"prob": e[:, 0].copy(), "alias": u[:, 1].copy(), "pmf_self": e[:, 2].copy(),
                "pmf_alias": e[:, 3].copy(), "entries": u.copy(), "weights": wt, "build_ms": ms.value}

    def set_light_grid(self, cells=8):
        """Per-shading-point light selection (rtg_set_light_grid): with set_light_sampling("power") active,
        the light of an NEE sample is picked from the alias table of the grid cell that holds the shading
        point, each light weighted by its power over its squared distance to the cell (0 where it faces
        away), mixed with uniform_share of the uniform pick. cells (1..64) is the number of cells on the
        longest axis of the scene's bounds; 0 turns it off (the default state). 8 is a stated choice, not
        an optimum (DESIGN.md 8l has the measurements). The same expectation as the other modes, with less
        noise where many similar lights are spread over the scene. The setting is kept whatever the light
        mode; frames that run the physical material model's, the path-MIS or the transmission kernels
        keep the power pick."""
        p = N.rtg_light_grid(int(cells))
        _check(self._lib.rtg_set_light_grid(self._h, C.byref(p)), self._lib.rtg_last_error)

    def light_grid(self):
        """The current setting and the active grid: {"cells", "active", "dims" (3,), "lo" (3,), "scale"
        (3,), "n_entries", "build_ms"} (dims, lo, scale as the kernel uses them; zeros when no grid is
        active)."""
        p = N.rtg_light_grid()
        _check(self._lib.rtg_get_light_grid(self._h, C.byref(p)), self._lib.rtg_last_error)
        dims, lo, sc = np.zeros(3, np.uint32), np.zeros(3, np.float32), np.zeros(3, np.float32)
        ne, ms = C.c_uint64(), C.c_double()
        _check(self._lib.rtg_light_grid_info(self._h, N.ptr(dims, C.c_uint32), N.ptr(lo, C.c_float),
                                             N.ptr(sc, C.c_float), C.byref(ne), C.byref(ms)), self._lib.rtg_last_error)
        return {"cells": int(p.cells), "active": ne.value != 0, "dims": dims, "lo": lo, "scale": sc,
                "n_entries": int(ne.value), "build_ms": ms.value}

    def light_grid_table(self):
        """The active grid's tables (rtg_light_grid_table): (cells, n_lights, 4) uint32, the words as the
        kernel loads them, cell c = (i_z * dims_y + i_y) * dims_x + i_x; None when no grid is active."""
        g = self.light_grid()
        if not g["active"]:
            return None
        e = np.zeros((g["n_entries"], 4), np.float32)
        _check(self._lib.rtg_light_grid_table(self._h, N.ptr(e, C.c_float)), self._lib.rtg_last_error)
        return e.view(np.uint32).reshape(-1, len(self.scene.lights), 4).copy()

    def light_grid_probe(self, points, r0, d1):
        """The shading kernel's own cell and pick (rtg_probe_light_grid) for points (n, 3) float32 and
        scripted draws r0 (n,) uint32, d1 (n,) float32 against the active grid: (cell (n,) int32, li (n,)
        int32, pmf (n,) float32)."""
        x = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        r = np.ascontiguousarray(r0, np.uint32).reshape(-1)
        d = np.ascontiguousarray(d1, np.float32).reshape(-1)
        if len(r) != len(d) or len(r) != len(x):
            raise ValueError("light_grid_probe: points, r0 and d1 must have one length")
        cell, li = np.zeros(len(r), np.int32), np.zeros(len(r), np.int32)
        pmf = np.zeros(len(r), np.float32)
        _check(self._lib.rtg_probe_light_grid(self._h, N.ptr(x, C.c_float), N.ptr(r, C.c_uint32), N.ptr(d, C.c_float),
                                              len(r), N.ptr(cell, C.c_int32), N.ptr(li, C.c_int32),
                                              N.ptr(pmf, C.c_float)), self._lib.rtg_last_error)
        return cell, li, pmf

    def set_material_model(self, mode="reference", transmission=False):
        """How conductor, plastic and Oren-Nayar materials shade (rtg_set_material_model). "reference"
        (default): as RTBase's stubs do, a cosine-sampled Lambertian, the reference's films bit for bit.
        "physical": a GGX conductor with the material's eta and k, a dielectric GGX coat over the diffuse
        base, and the qualitative Oren-Nayar model (include/rtg.h has the definition); a lobe narrower
        than RTG_ALPHA_DELTA reflects as a mirror. The scene's own parameters (Scene.material_params) are
        handed to the library here. Applies to render(), adaptiveRender() and the "path" and "direct"
        integrators; "direct_mis", "albedo", "normals", lightTracer(), instantRadiosity() and the
        denoiser's guides keep the reference model. A scene without such a material renders the same
        film under both. transmission=True (with "physical" only) hands the library
        Scene.material_params_transmissive instead: the scene's rough dielectrics shade with GGX reflection
        and refraction (RTG_MODEL_ROUGH_DIELECTRIC) in place of the Lambertian stub; False is the call as it
        was, record for record, and a change of the choice hands the other set."""
        m = _material_model(mode)
        _material_params_choice(self, m, transmission, self._lib.rtg_set_material_params, self._h)
        _check(self._lib.rtg_set_material_model(self._h, m), self._lib.rtg_last_error)

    def material_model(self):
        """The current setting, "reference" or "physical"."""
        m = C.c_int()
        _check(self._lib.rtg_get_material_model(self._h, C.byref(m)), self._lib.rtg_last_error)
        return {v: k for k, v in MATERIAL_MODELS.items()}.get(m.value, m.value)

    material_probe = staticmethod(material_probe)
    transmission_probe = staticmethod(transmission_probe)

    def set_path_mis(self, mode="off"):
        """Multiple importance sampling of emitters in the path tracer (rtg_set_path_mis). "off"
        (default): pathTrace as the reference has it, NEE alone after a non-specular bounce and the
        background unweighted on a miss, the reference's films bit for bit. "power": the NEE sample and the
        BSDF sample of every non-specular vertex are combined with the power heuristic, and a miss is
        weighted by the path throughput (include/rtg.h has the definition): the same paths as "off" for
        the same seed, other weights; the correct estimator under an environment light, where "off"
        counts the environment twice. Applies to render(), adaptiveRender() and the "path" integrator
        only, with every environment, light selection, material and camera setting; not to "direct",
        "direct_mis", "albedo", "normals", lightTracer(), instantRadiosity() or the denoiser's guides."""
        _check(self._lib.rtg_set_path_mis(self._h, _path_mis(mode)), self._lib.rtg_last_error)

    def path_mis(self):
        """The current setting, "off" or "power"."""
        m = C.c_int()
        _check(self._lib.rtg_get_path_mis(self._h, C.byref(m)), self._lib.rtg_last_error)
        return {v: k for k, v in PATH_MIS.items()}.get(m.value, m.value)

    mis_weight_probe = staticmethod(mis_weight_probe)

    def set_sampler(self, name="pcg"):
        """Where the random numbers of a path and of a camera sample come from (rtg_set_sampler). "pcg"
        (default): one PCG32 stream per (pixel, sample), today's films bit for bit. "sobol": Burley's
        hash-based Owen-scrambled Sobol sequence, padded 4-D (include/rtg.h has the definition): the
        samples of a pixel are stratified against each other in every group of four draws; no estimator
        changes. Applies to render(), adaptiveRender() and the "path", "direct" and "direct_mis"
        integrators, with either environment mode, the uniform and power light picks and camera sampling;
        frames under the light grid, the physical material model or path MIS keep "pcg", as
        lightTracer() and instantRadiosity() do (sampler_active tells)."""
        _check(self._lib.rtg_set_sampler(self._h, _sampler(name)), self._lib.rtg_last_error)

    @property
    def sampler(self):
        """The current setting, "pcg" or "sobol"."""
        m = C.c_int()
        _check(self._lib.rtg_get_sampler(self._h, C.byref(m)), self._lib.rtg_last_error)
        return {v: k for k, v in SAMPLERS.items()}.get(m.value, m.value)

    @property
    def sampler_active(self):
        """What the next render() would draw from under the handle's other settings (rtg_sampler_active)."""
        m = C.c_int()
        _check(self._lib.rtg_sampler_active(self._h, C.byref(m)), self._lib.rtg_last_error)
        return {v: k for k, v in SAMPLERS.items()}.get(m.value, m.value)

    def env_pdf(self, dirs):
        """The solid-angle density the current environment mode gives directions (n, 3)
        (rtg_probe_env_pdf): the luminance table's cell density over sin theta, or 1 / (4 pi)."""
        d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        out = np.zeros(len(d), np.float32)
        _check(self._lib.rtg_probe_env_pdf(self._h, N.ptr(d, C.c_float), len(d), N.ptr(out, C.c_float)),
               self._lib.rtg_last_error)
        return out

    def light_of_triangle(self):
        """The triangle -> light map of set_path_mis("power") (rtg_light_of_triangle): (n_triangles,)
        int32, the triangle's index in Scene.lights or -1."""
        out = np.zeros(self.scene.desc.n_tris, np.int32)
        _check(self._lib.rtg_light_of_triangle(self._h, N.ptr(out, C.c_int32)), self._lib.rtg_last_error)
        return out

    def light_records(self):
        """The light records as uploaded (rtg_light_records): (n_lights, 20) float32 = v0.xyz area |
        v1.xyz type bits (0 area, 1 environment) | v2.xyz 1/area | geometric normal.xyz - | emission.rgb -."""
        out = np.zeros((len(self.scene.lights), 20), np.float32)
        _check(self._lib.rtg_light_records(self._h, N.ptr(out, C.c_float)), self._lib.rtg_last_error)
        return out

    def light_picks(self, r0, d1):
        """The shading kernel's own light pick (rtg_probe_light_pick) for scripted draws r0 (n,) uint32
        and d1 (n,) float32 against the active table: (li (n,) int32, pmf (n,) float32)."""
        r = np.ascontiguousarray(r0, np.uint32).reshape(-1)
        d = np.ascontiguousarray(d1, np.float32).reshape(-1)
        if len(r) != len(d):
            raise ValueError("light_picks: r0 and d1 must have one length")
        li = np.zeros(len(r), np.int32)
        pmf = np.zeros(len(r), np.float32)
        _check(self._lib.rtg_probe_light_pick(self._h, N.ptr(r, C.c_uint32), N.ptr(d, C.c_float), len(r),
                                              N.ptr(li, C.c_int32), N.ptr(pmf, C.c_float)), self._lib.rtg_last_error)
        return li, pmf

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.rtg_destroy(h)

    def set_options(self, max_depth=None, flags=None, max_paths=0):
        if max_depth is not None:
            self.max_depth = max_depth
        if flags is not None:
            self.flags = flags
        _check(self._lib.rtg_set_options(self._h, self.max_depth, self.flags, max_paths), self._lib.rtg_last_error)

    @property
    def handle(self):
        """The rtg_handle* (ctypes void pointer) for direct C-ABI calls (e.g. rtg_film_gather)."""
        return self._h

    @property
    def tiles_x(self):
        return (self.width + 31) // 32

    @property
    def tiles_y(self):
        return (self.height + 31) // 32

    def render(self, n_samples=1, tiles=None, first_sample=None, sync=True, stream=None):
        """RayTracer::render(): add n_samples samples per pixel (default 1 = one frame).
        sync=False queues the frame (rtg_render_async): a frame loop of 1-spp calls then keeps up to
        three frames in flight on the GPU; film() / stats() / synchronize() wait for them.
        stream (a HIP stream handle, not the null stream): the render is ordered after the caller's
        earlier work on that stream and the caller's later work on it sees the film; the call returns
        without waiting (rtg_render_async with a stream)."""
        first = self.getSPP() if first_sample is None else first_sample
        t = None if tiles is None else np.ascontiguousarray(tiles, np.uint32)
        tp = N.ptr(t, C.c_uint32) if t is not None else None
        nt = 0 if t is None else len(t)
        if stream:
            rc = self._lib.rtg_render_async(self._h, first, n_samples, self.seed, tp, nt, C.c_void_p(stream))
        elif sync:
            rc = self._lib.rtg_render(self._h, first, n_samples, self.seed, tp, nt)
        else:
            rc = self._lib.rtg_render_async(self._h, first, n_samples, self.seed, tp, nt, None)
        _check(rc, self._lib.rtg_last_error)

    def adaptiveRender(self, init_samples=2, max_samples=10240, min_samples=1, first_sample=None):
        """RayTracer::adaptiveRender (Renderer.h:583-749): one frame whose per-tile sample counts
        follow the tiles' variance after init_samples samples. Returns the per-tile counts. The frame
        draws sample indices first_sample ... first_sample + init_samples + max(count) - 1 of the
        PCG streams keyed by `seed` (limit: RTG_MAX_SAMPLES_PER_KEY = 65536). Default (first_sample
        None): frame f = getSPP() draws indices 0 ... of its own seed, seed + f * 0x9E3779B97F4A7C15
        (mod 2^64), so any number of frames stays inside the key space."""
        if first_sample is None:
            first, seed = 0, (self.seed + self.getSPP() * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
        else:
            first, seed = first_sample, self.seed
        counts = np.zeros(self.tiles_x * self.tiles_y, np.uint32)
        _check(self._lib.rtg_render_adaptive(self._h, first, seed, init_samples, max_samples, min_samples,
                                             N.ptr(counts, C.c_uint32)), self._lib.rtg_last_error)
        return counts

    def lightTracer(self, n_frames=1, first_frame=None):
        """RayTracer::lightTracer (Renderer.h:221-326): width*height light paths per frame, each
        vertex connected to the camera and splatted (Film::SPP += 1 per frame)."""
        first = self.getSPP() if first_frame is None else first_frame
        _check(self._lib.rtg_render_light(self._h, first, n_frames, self.seed), self._lib.rtg_last_error)

    def instantRadiosity(self, n_frames=1, n_vpl=50, first_frame=None):
        """RayTracer::instantRadiosity (Renderer.h:82-218): n_vpl VPL paths (MAX_VPL = 50) per frame,
        then every pixel's first hit gathers all visible VPLs (Film::SPP += 1 per frame)."""
        first = self.getSPP() if first_frame is None else first_frame
        _check(self._lib.rtg_render_instant_radiosity(self._h, first, n_frames, self.seed, n_vpl),
               self._lib.rtg_last_error)

    def connect_probe(self, points, normals, colours):
        """The light tracer's own connectToCamera on this tracer's camera, apart from its visibility
        test (rtg_probe_connect, test surface), for n points, shading normals and colours ((n, 3) each).
        Returns (n, 12) float32: accepted and pixel as int32 bits, the splatted colour, the shadow
        ray's origin, maxT and direction; all zero where the connection is not accepted."""
        p, nn, c = (np.ascontiguousarray(v, np.float32).reshape(-1, 3) for v in (points, normals, colours))
        if not len(p) == len(nn) == len(c):
            raise ValueError("connect_probe: points, normals and colours must have one length")
        out = np.zeros((len(p), 12), np.float32)
        _check(self._lib.rtg_probe_connect(self._h, N.ptr(p, C.c_float), N.ptr(nn, C.c_float), N.ptr(c, C.c_float),
                                           len(p), N.ptr(out, C.c_float)), self._lib.rtg_last_error)
        return out

    def synchronize(self):
        _check(self._lib.rtg_synchronize(self._h), self._lib.rtg_last_error)

    def idle(self):
        """True when no queued render work is left on the GPU (rtg_render_idle)."""
        v = C.c_int()
        _check(self._lib.rtg_render_idle(self._h, C.byref(v)), self._lib.rtg_last_error)
        return bool(v.value)

    def film(self):
        """(sum, spp): the unnormalised Film::film and Film::SPP."""
        out = np.zeros((self.height, self.width, 3), np.float32)
        spp = C.c_uint32()
        _check(self._lib.rtg_film_read(self._h, N.ptr(out, C.c_float), C.byref(spp)), self._lib.rtg_last_error)
        return out, spp.value

    def load_film(self, film_sum, spp):
        f = np.ascontiguousarray(film_sum, np.float32)
        _check(self._lib.rtg_film_load(self._h, N.ptr(f, C.c_float), spp), self._lib.rtg_last_error)

    def copy_film_to(self, device_ptr):
        _check(self._lib.rtg_film_copy_device(self._h, C.c_void_p(device_ptr)), self._lib.rtg_last_error)

    def getSPP(self):
        spp = C.c_uint32()
        _check(self._lib.rtg_film_read(self._h, None, C.byref(spp)), self._lib.rtg_last_error)
        return spp.value

    def clear(self):
        _check(self._lib.rtg_clear(self._h), self._lib.rtg_last_error)

    def saveHDR(self, filename):
        f, spp = self.film()
        save_hdr(filename, f, max(spp, 1))

    def savePNG(self, filename):
        f, spp = self.film()
        save_png(filename, f, spp)

    def denoise(self, iterations=5, normal_squarings=5, sigma_colour=1.0, sigma_albedo=0.1):
        """The counterpart of RayTracer::denoise (Renderer.h:752-793, OIDN, never called by the
        reference): film / SPP filtered on the GPU by the project's own edge-avoiding a-trous
        wavelet filter, guided by the scene's albedo and shading normals (rtg_denoise; not a
        reproduction of OIDN's output). Returns the (H, W, 3) float32 mean image; the film, SPP and
        the settings stay as they were. Waits for queued frames first."""
        out = np.zeros((self.height, self.width, 3), np.float32)
        p = _denoise_params(iterations, normal_squarings, sigma_colour, sigma_albedo)
        _check(self._lib.rtg_denoise(self._h, C.byref(p), N.ptr(out, C.c_float)), self._lib.rtg_last_error)
        return out

    def guides(self):
        """(albedo, normals): the denoiser's guide images, 1 sample of the "albedo" and "normals"
        integrators each, rendered once per RayTracer and cached (rtg_denoise_guides)."""
        a = np.zeros((self.height, self.width, 3), np.float32)
        n = np.zeros((self.height, self.width, 3), np.float32)
        _check(self._lib.rtg_denoise_guides(self._h, N.ptr(a, C.c_float), N.ptr(n, C.c_float)),
               self._lib.rtg_last_error)
        return a, n

    def copy_denoised_to(self, device_ptr):
        """The last denoise() result, (H, W, 3) float32, copied to device memory on this GPU
        (rtg_denoise_copy_device; like copy_film_to)."""
        _check(self._lib.rtg_denoise_copy_device(self._h, C.c_void_p(device_ptr)), self._lib.rtg_last_error)

    def denoise_ms(self):
        """Device time of the last denoise() (pack, iterations, unpack), in ms."""
        return self._lib.rtg_denoise_ms(self._h)

    def stats(self):
        s = N.rtg_stats()
        _check(self._lib.rtg_get_stats(self._h, C.byref(s)), self._lib.rtg_last_error)
        return {k: getattr(s, k) for k, _ in N.rtg_stats._fields_}

    def trace_closest(self, rays):
        r = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        out = np.zeros((len(r), 4), np.float32)
        _check(self._lib.rtg_trace_closest(self._h, N.ptr(r, C.c_float), len(r), N.ptr(out, C.c_float)),
               self._lib.rtg_last_error)
        return out

    def trace_visible(self, rays):
        r = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        out = np.zeros(len(r), np.int32)
        _check(self._lib.rtg_trace_visible(self._h, N.ptr(r, C.c_float), len(r), N.ptr(out, C.c_int32)),
               self._lib.rtg_last_error)
        return out


class RayTracerGroup:
    """RayTracer over several GPUs of one node (rtg_group_*, rtg_multi.hip): rank r renders the 32x32
    tiles with (tile_x + tile_y) % N == r on devices[r] (one host thread per device), and film()
    assembles the film on devices[0] from every rank's own tiles (packed on each device, one RCCL
    send per rank, scattered on devices[0]). The result is bit-identical to a one-device render
    (RayTracer::pathTracerTileBased's tile pool, Renderer.h:836-853, spread over devices). A device
    list with repeats rehearses N ranks on fewer GPUs (the ranks then render in turn and the packed
    tiles move with device copies)."""

    def __init__(self, scene, devices=(0,), max_depth=RayTracer.MAX_DEPTH, seed=1234, cull=True, max_paths=0):
        self.scene = scene
        self.seed = seed
        self.devices = list(devices)
        self.width, self.height = scene.width, scene.height
        self._lib = N.rtg()
        dev = np.ascontiguousarray(self.devices, np.int32)
        g = C.c_void_p()
        _check(self._lib.rtg_group_create(N.ptr(dev, C.c_int32), len(dev), scene.desc_ptr, C.byref(g)),
               self._lib.rtg_last_error)
        self._g = g
        self.max_depth = max_depth
        self.flags = N.RTG_OPT_CULL if cull else 0
        _check(self._lib.rtg_group_set_options(g, max_depth, self.flags, max_paths), self._lib.rtg_last_error)
        self._spp = 0

    def set_options(self, max_depth=None, flags=None, max_paths=0):
        if max_depth is not None:
            self.max_depth = max_depth
        if flags is not None:
            self.flags = flags
        _check(self._lib.rtg_group_set_options(self._g, self.max_depth, self.flags, max_paths),
               self._lib.rtg_last_error)

    def set_camera_sampling(self, filter="none", filter_radius=None, lens_radius=0.0, focal_distance=1.0):
        """RayTracer.set_camera_sampling on every rank (rtg_group_set_camera_sampling)."""
        p = _camera_sampling(filter, filter_radius, lens_radius, focal_distance)
        _check(self._lib.rtg_group_set_camera_sampling(self._g, C.byref(p)), self._lib.rtg_last_error)

    def set_camera(self, camera, projection):
        """RayTracer.set_camera on every rank (rtg_group_set_camera)."""
        _check(self._lib.rtg_group_set_camera(self._g, C.byref(camera), C.byref(projection)), self._lib.rtg_last_error)

    def set_env_sampling(self, mode="uniform"):
        """RayTracer.set_env_sampling on every rank (rtg_group_set_env_sampling)."""
        _check(self._lib.rtg_group_set_env_sampling(self._g, _env_mode(mode)), self._lib.rtg_last_error)

    def set_light_sampling(self, mode="uniform", uniform_share=0.125):
        """RayTracer.set_light_sampling on every rank (rtg_group_set_light_sampling)."""
        p = _light_sampling(mode, uniform_share)
        _check(self._lib.rtg_group_set_light_sampling(self._g, C.byref(p)), self._lib.rtg_last_error)

    def set_light_grid(self, cells=8):
        """RayTracer.set_light_grid on every rank (rtg_group_set_light_grid)."""
        p = N.rtg_light_grid(int(cells))
        _check(self._lib.rtg_group_set_light_grid(self._g, C.byref(p)), self._lib.rtg_last_error)

    def set_path_mis(self, mode="off"):
        """RayTracer.set_path_mis on every rank (rtg_group_set_path_mis)."""
        _check(self._lib.rtg_group_set_path_mis(self._g, _path_mis(mode)), self._lib.rtg_last_error)

    def set_sampler(self, name="pcg"):
        """RayTracer.set_sampler on every rank (rtg_group_set_sampler)."""
        _check(self._lib.rtg_group_set_sampler(self._g, _sampler(name)), self._lib.rtg_last_error)

    def set_material_model(self, mode="reference", transmission=False):
        """RayTracer.set_material_model on every rank (rtg_group_set_material_params / _model)."""
        m = _material_model(mode)
        _material_params_choice(self, m, transmission, self._lib.rtg_group_set_material_params, self._g)
        _check(self._lib.rtg_group_set_material_model(self._g, m), self._lib.rtg_last_error)

    def setup_ms(self):
        """(host build of the device records, parallel uploads) of rtg_group_create, in ms."""
        a, b = C.c_double(), C.c_double()
        _check(self._lib.rtg_group_setup_ms(self._g, C.byref(a), C.byref(b)), self._lib.rtg_last_error)
        return a.value, b.value

    def reduce(self, sync=True):
        """Assemble the film on devices[0] from every rank's own tiles (RCCL send/recv; device copies
        for repeated devices). sync=False queues it on the exchange streams after every rank's queued
        frames (rtg_group_reduce_async): the ranks' next frames run on meanwhile."""
        fn = self._lib.rtg_group_reduce if sync else self._lib.rtg_group_reduce_async
        _check(fn(self._g), self._lib.rtg_last_error)

    def synchronize(self):
        """Wait for every rank's queued frames and the queued exchanges (rtg_group_synchronize)."""
        _check(self._lib.rtg_group_synchronize(self._g), self._lib.rtg_last_error)

    def rank_stats(self):
        """rtg_get_stats of every rank's handle (rays, kernel ms, counting-pass counters)."""
        out = []
        for r in range(len(self.devices)):
            h = self._lib.rtg_group_handle(self._g, r)
            st = N.rtg_stats()
            _check(self._lib.rtg_get_stats(h, C.byref(st)), self._lib.rtg_last_error)
            out.append({k: getattr(st, k) for k, _ in N.rtg_stats._fields_})
        return out

    def __del__(self):
        g, self._g = getattr(self, "_g", None), None
        if g:
            self._lib.rtg_group_destroy(g)

    @property
    def uses_rccl(self):
        return bool(self._lib.rtg_group_uses_rccl(self._g))

    def render(self, n_samples=1, first_sample=None, sync=True):
        """Every rank adds n_samples samples of its tiles. sync=False queues the frame on every rank
        (rtg_group_render_async: coalesced and pipelined per rank, as RayTracer.render(sync=False))."""
        first = self._spp if first_sample is None else first_sample
        fn = self._lib.rtg_group_render if sync else self._lib.rtg_group_render_async
        _check(fn(self._g, first, n_samples, self.seed), self._lib.rtg_last_error)
        self._spp = first + n_samples

    def film(self):
        """(sum, spp) of the reduced film."""
        out = np.zeros((self.height, self.width, 3), np.float32)
        spp = C.c_uint32()
        _check(self._lib.rtg_group_film_read(self._g, N.ptr(out, C.c_float), C.byref(spp)), self._lib.rtg_last_error)
        return out, spp.value

    def denoise(self, iterations=5, normal_squarings=5, sigma_colour=1.0, sigma_albedo=0.1):
        """RayTracer.denoise() of the assembled film (reduced first if needed), filtered on devices[0]
        with rank 0's guides (rtg_group_denoise): (H, W, 3) float32, bit-identical to one device's."""
        out = np.zeros((self.height, self.width, 3), np.float32)
        p = _denoise_params(iterations, normal_squarings, sigma_colour, sigma_albedo)
        _check(self._lib.rtg_group_denoise(self._g, C.byref(p), N.ptr(out, C.c_float)), self._lib.rtg_last_error)
        return out

    def reduce_ms(self):
        return self._lib.rtg_group_reduce_ms(self._g)

    def clear(self):
        _check(self._lib.rtg_group_clear(self._g), self._lib.rtg_last_error)
        self._spp = 0


def tiles_for_rank_native(width, height, rank, world):
    """rtg_tiles_for_rank (the C partition the group uses); equals distributed.tiles_for_rank."""
    lib = N.rtg()
    n = C.c_uint32()
    _check(lib.rtg_tiles_for_rank(width, height, rank, world, None, C.byref(n)), lib.rtg_last_error)
    out = np.zeros(n.value, np.uint32)
    _check(lib.rtg_tiles_for_rank(width, height, rank, world, N.ptr(out, C.c_uint32), C.byref(n)), lib.rtg_last_error)
    return out
