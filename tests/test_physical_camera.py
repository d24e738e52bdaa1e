"""Physical camera: camera rays traced through a lens of spherical interfaces (cuda/camera_physical.cuh; luminary_amd/csrc/device/dev_camera.h).

The checker is tests/support/physical_camera_check.c, a plain-C restatement of the exact flavour's camera ray; it takes its random numbers and
sin/cos from the test oracle. The CPU tests pin the host API, the default lens and the restatement itself (against an independent float64
vector-Snell trace); the GPU tests hold the device to the restatement bit for bit and check what the renderer does with the rays."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import oracle_lib
from luminary_amd import CameraLens, Host, LuminaryError, default_material, scenes
from luminary_amd.core import Core, PhysicalCamera, CNT_TRACE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "physical_camera_lens.json")
FLT_MAX = float(np.finfo(np.float32).max)
W, H = 48, 32


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


_CHECK = {}


def _check_lib(tmp_path_factory):
    """tests/support/physical_camera_check.c, built like the other C checkers (no contraction), linked against the oracle library."""
    if "lib" not in _CHECK:
        oracle = oracle_lib.lib()  # builds oracle/_build/liboracle.so if needed
        d = tmp_path_factory.mktemp("pc_check")
        so = str(d / "physical_camera_check.so")
        build = os.path.join(ROOT, "oracle", "_build")
        subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-fPIC", "-shared", os.path.join(ROOT, "tests", "support", "physical_camera_check.c"),
                               "-o", so, "-L", build, "-loracle", "-Wl,-rpath," + build, "-lm"])
        lib = C.CDLL(so)
        lib.pc_lens_walk.restype = C.c_float
        lib.pc_sensor_sample.restype = C.c_float
        _CHECK["lib"], _CHECK["oracle"] = lib, oracle
    return _CHECK["lib"]


def _physical_camera(lens_json=None, reflections=False, camera=None):
    """The converted camera (device_structs.c:40-72) of the reference's default physical parameters and a lens table."""
    host = Host()
    try:
        c = camera or host.get_camera()
    finally:
        host.close()
    g = lens_json or _golden()
    p = PhysicalCamera()
    ph = c.physical
    p.aperture_point, p.aperture_radius = ph.aperture_point, np.float32(ph.aperture_diameter) * np.float32(0.5)
    p.exit_pupil_point, p.exit_pupil_radius = ph.exit_pupil_point, np.float32(ph.exit_pupil_diameter) * np.float32(0.5)
    p.image_plane_distance, p.sensor_width = ph.image_plane_distance, ph.sensor_width
    p.allow_reflections = 1 if reflections else 0
    p.num_interfaces = len(g["interfaces"])
    for i, (r, v, cy) in enumerate(g["interfaces"]):
        p.interfaces[i].radius, p.interfaces[i].vertex, p.interfaces[i].cylindrical_radius = r, v, cy
    for i, (n, a, cy) in enumerate(g["media"]):
        p.media[i].design_ior, p.media[i].abbe, p.media[i].cylindrical_radius = n, a, cy
    return p


def _restated_rays(lib, pc, width, height, pos, rot, scale, pixels, first, samples):
    px = np.ascontiguousarray(pixels, dtype=np.uint32)
    n = px.size * samples
    o, d, w = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32), np.zeros(n, np.float32)
    bn = oracle_lib.bluenoise()
    pos = (C.c_float * 3)(*pos)
    rot = (C.c_float * 4)(*rot)
    lib.pc_camera_rays(C.byref(pc), bn.ctypes.data_as(C.c_void_p), C.c_uint32(width), C.c_uint32(height), pos, rot, C.c_float(scale),
                       px.ctypes.data_as(C.c_void_p), C.c_uint32(px.size), C.c_uint32(first), C.c_uint32(samples), o.ctypes.data_as(C.c_void_p),
                       d.ctypes.data_as(C.c_void_p), w.ctypes.data_as(C.c_void_p))
    return o, d, w


# ---------------------------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------------------------

def test_physical_camera_builds_and_spectral_rendering_is_refused(capfd):
    host = Host()
    try:
        c = host.get_camera()
        c.use_physical_camera = True
        host.set_camera(c)
        host.device_scene()  # the scope error of the thin-lens-only renderer is gone
        c.physical.use_spectral_rendering = True
        host.set_camera(c)
        with pytest.raises(LuminaryError):
            host.device_scene()
        assert "spectral rendering" in capfd.readouterr().err
        c.physical.use_spectral_rendering = False
        c.physical.exit_pupil_diameter = 0.0
        host.set_camera(c)
        with pytest.raises(LuminaryError):
            host.device_scene()
    finally:
        host.close()


def _lens_table(lens):
    n = lens.num_interfaces
    return ([[lens.interfaces[i].radius, lens.interfaces[i].vertex, lens.interfaces[i].cylindrical_radius] for i in range(n)],
            [[lens.media[i].design_ior, lens.media[i].abbe, lens.media[i].cylindrical_radius] for i in range(n + 1)])


def test_default_lens_round_trip_validation_and_restart():
    from luminary_amd import _lib
    g = _golden()
    host = Host()
    try:
        lens = host.get_camera_lens()
        iface, media = _lens_table(lens)
        assert lens.num_interfaces == 12
        assert np.array_equal(np.float32(iface), np.float32(g["interfaces"])), "the reference's prescription, scaled in float32"
        assert np.array_equal(np.float32(media), np.float32(g["media"]))
        # set / get
        mine = CameraLens()
        mine.num_interfaces = 2
        for i, (r, v, cy) in enumerate([(30.0, 0.0, 8.0), (-30.0, 4.0, 8.0)]):
            mine.interfaces[i].radius, mine.interfaces[i].vertex, mine.interfaces[i].cylindrical_radius = r, v, cy
        for i, (n, a, cy) in enumerate([(1.0003, 0.0, FLT_MAX), (1.5, 60.0, 8.0), (1.0003, 0.0, FLT_MAX)]):
            mine.media[i].design_ior, mine.media[i].abbe, mine.media[i].cylindrical_radius = n, a, cy
        host.set_camera_lens(mine)
        assert _lens_table(host.get_camera_lens()) == _lens_table(mine)
        # validation
        for bad in ("count0", "count25", "nan", "inf", "ior0"):
            b = CameraLens()
            C.memmove(C.byref(b), C.byref(mine), C.sizeof(CameraLens))
            if bad == "count0":
                b.num_interfaces = 0
            elif bad == "count25":
                b.num_interfaces = 25
            elif bad == "nan":
                b.interfaces[1].radius = float("nan")
            elif bad == "inf":
                b.media[1].design_ior = float("inf")
            else:
                b.media[1].design_ior = 0.0
            with pytest.raises(LuminaryError):
                host.set_camera_lens(b)
        assert _lens_table(host.get_camera_lens()) == _lens_table(mine), "a refused lens changes nothing"
        # a lens change restarts the integration (entity 2); an equal lens does not
        fn = _lib().luminary_ext_change_restarts_integration
        fn.restype = C.c_uint64
        out = C.c_bool()
        assert fn(2, C.byref(mine), C.byref(lens), C.byref(out)) == 0 and out.value
        assert fn(2, C.byref(mine), C.byref(mine), C.byref(out)) == 0 and not out.value
    finally:
        host.close()


def _snell_trace_f64(g, o, d):
    """Independent float64 trace of the lens without reflections: vector Snell at every interface, aperture stop and rims. Returns the end point, the
    direction, the Fresnel transmission product, a validity mask and a mask of rays that pass within 1e-4 mm of an aperture or rim edge (or reach a
    glass element's cylindrical wall, which the model reflects off and this trace does not follow)."""
    pc = _physical_camera(g)
    o, d = o.astype(np.float64).copy(), d.astype(np.float64).copy()
    n = len(o)
    alive = np.ones(n, bool)
    edge = np.zeros(n, bool)
    wgt = np.ones(n)
    ior = np.full(n, 1.0003)
    cyl = np.full(n, np.inf)
    ap_z, ap_r = float(np.float32(pc.aperture_point)), float(np.float32(pc.aperture_radius))
    for i, (R, V, CR) in enumerate(g["interfaces"]):
        m = g["media"][i + 1]
        cz = V - R
        oc = o - np.array([0, 0, cz])
        b = np.sum(oc * d, 1)
        c = np.sum(oc * oc, 1) - R * R
        disc = b * b - c
        hit = disc >= 0
        sq = np.sqrt(np.maximum(disc, 0))
        t0, t1 = -b - sq, -b + sq
        t = np.where(t0 > 0, t0, t1)
        hit &= t > 0
        # the cylindrical wall of the medium the ray is in (glass only)
        rxy = np.hypot(d[:, 0], d[:, 1])
        with np.errstate(divide="ignore", invalid="ignore"):
            a2 = d[:, 0] ** 2 + d[:, 1] ** 2
            bb = o[:, 0] * d[:, 0] + o[:, 1] * d[:, 1]
            cc = o[:, 0] ** 2 + o[:, 1] ** 2 - cyl ** 2
            tw = (-bb + np.sqrt(np.maximum(bb * bb - a2 * cc, 0))) / a2
        wall = np.isfinite(cyl) & (rxy > 0) & (tw > 0) & (tw < t + 1e-4)
        edge |= alive & wall
        # aperture stop
        with np.errstate(divide="ignore", invalid="ignore"):
            ta = (ap_z - o[:, 2]) / d[:, 2]
        pa = o + d * ta[:, None]
        ra = np.hypot(pa[:, 0], pa[:, 1])
        crosses = (ta > 0) & (ta < t)
        blocked = crosses & (ra > ap_r)
        edge |= alive & crosses & (np.abs(ra - ap_r) < 1e-4)
        p = o + d * t[:, None]
        rp = np.hypot(p[:, 0], p[:, 1])
        edge |= alive & hit & (np.abs(rp - CR) < 1e-4)
        alive &= hit & ~blocked & (rp <= CR)
        nrm = (p - np.array([0, 0, cz])) / abs(R)
        nrm = np.where((np.sum(nrm * d, 1) > 0)[:, None], -nrm, nrm)  # against the ray
        eta = ior / m[0]
        cosi = -np.sum(nrm * d, 1)
        k = 1 - eta * eta * (1 - cosi * cosi)
        tir = k < 0
        alive &= ~tir
        cost = np.sqrt(np.maximum(k, 0))
        dt = eta[:, None] * d + (eta * cosi - cost)[:, None] * nrm
        with np.errstate(divide="ignore", invalid="ignore"):  # (rays that are already dead)
            rs = ((eta * cosi - cost) / (eta * cosi + cost)) ** 2
            rp_ = ((eta * cost - cosi) / (eta * cost + cosi)) ** 2
        wgt *= np.where(alive, 1 - 0.5 * (rs + rp_), 1.0)
        o, d = np.where(alive[:, None], p, o), np.where(alive[:, None], dt / np.linalg.norm(dt, axis=1)[:, None], d)
        ior = np.where(alive, m[0], ior)
        cyl = np.where(alive, m[2] if m[2] < 1e30 else np.inf, cyl)
    return o, d, wgt, alive, edge


def test_restated_walk_matches_a_float64_snell_trace(tmp_path_factory):
    lib = _check_lib(tmp_path_factory)
    g = _golden()
    pc = _physical_camera(g)
    bn = oracle_lib.bluenoise()
    rng = np.random.default_rng(5)
    N = 10000
    o = np.zeros((N, 3), np.float32)
    d = np.zeros((N, 3), np.float32)
    # sensor points over the sensor and exit-pupil targets over the pupil, as the camera draws them
    sx = rng.uniform(-pc.sensor_width, pc.sensor_width, N)
    sy = rng.uniform(-pc.sensor_width * 2 / 3, pc.sensor_width * 2 / 3, N)
    a, r = rng.uniform(0, 2 * np.pi, N), np.sqrt(rng.uniform(0, 1, N)) * pc.exit_pupil_radius
    o[:] = np.stack([sx, sy, np.full(N, -pc.image_plane_distance)], 1)
    tgt = np.stack([np.cos(a) * r, np.sin(a) * r, np.full(N, pc.exit_pupil_point)], 1)
    d[:] = (tgt - o) / np.linalg.norm(tgt - o, axis=1)[:, None]
    eo, ed, ew = o.copy(), d.copy(), np.zeros(N, np.float32)
    for i in range(N):
        oi, di = (C.c_float * 3)(*eo[i]), (C.c_float * 3)(*ed[i])
        ew[i] = lib.pc_lens_walk(C.byref(pc), bn.ctypes.data_as(C.c_void_p), 0, 0, 0, oi, di)
        eo[i], ed[i] = list(oi), list(di)
    fo, fd, fw, alive, edge = _snell_trace_f64(g, o, d)
    valid = ew > 0
    keep = ~edge
    assert keep.mean() > 0.5
    assert np.array_equal(valid[keep], alive[keep]), "validity agrees away from the aperture's and the rims' edges"
    both = keep & valid & alive
    assert both.sum() > 1000
    rel = lambda x, y: np.abs(x - y) / np.maximum(np.abs(y), 1.0)
    assert rel(eo[both], fo[both]).max() < 1e-4 and rel(ed[both], fd[both]).max() < 1e-4
    assert (np.abs(ew[both] - fw[both]) / fw[both]).max() < 1e-4


def test_paraxial_focal_length_of_the_default_lens():
    """Reported, not gated: the effective focal length of the default lens from a float64 ray-transfer trace (the reference scales its prescription to
    50.53 mm)."""
    g = _golden()
    M = np.eye(2)
    n1 = g["media"][0][0]
    z = g["interfaces"][0][1]
    for i, (R, V, _) in enumerate(g["interfaces"]):
        M = np.array([[1, V - z], [0, 1]]) @ M
        n2 = g["media"][i + 1][0]
        M = np.array([[1, 0], [-(n2 - n1) / (n2 * R), n1 / n2]]) @ M
        n1, z = n2, V
    efl = -1.0 / M[1, 0]
    print("paraxial effective focal length of the default lens: %.3f mm" % efl)
    assert np.isfinite(efl)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------------------------

def _host(width=W, height=H, depth=1, sky=(0.75, 0.5, 0.25), reflections=False, plane_z=None, pos=(0.0, 0.0, 0.0), rot=(0.0, 0.0, 0.0), scale=1.0):
    """A constant-sky scene behind a physical camera; one quad either far behind the camera (sky only) or as a wall at z = plane_z."""
    host = Host()
    scenes.apply_benchmark_settings(host, width, height, depth, sky=sky)
    mat = host.add_material(default_material())
    z = 50.0 if plane_z is None else plane_z
    q = np.float32([[-20, -20, z], [20, -20, z], [20, 20, z], [-20, -20, z], [20, 20, z], [-20, 20, z]])
    mesh = host.add_mesh(q.reshape(-1), np.full(2, mat, np.uint16))
    host.new_instance(mesh)
    scenes.set_camera(host, pos, rot)
    c = host.get_camera()
    c.use_physical_camera = True
    c.physical.allow_reflections = reflections
    c.camera_scale = scale
    host.set_camera(c)
    return host


def _core_for(host, reflections=False, lens=None):
    view = oracle_lib.with_luts(host.device_scene())
    core = Core(0)
    core.upload(view)
    core.set_physical_camera(_physical_camera(lens, reflections, host.get_camera()))
    return core, view


@pytest.mark.gpu
@pytest.mark.parametrize("reflections", [False, True])
def test_device_rays_equal_the_restatement(tmp_path_factory, reflections):
    lib = _check_lib(tmp_path_factory)
    total = 0
    for pos, rot, scale in (((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 1.0), ((1.5, -2.0, 3.0), (0.3, -0.7, 0.2), 4.0), ((-3.0, 1.0, 0.5), (1.2, 2.5, -0.4), 0.25)):
        host = _host(96, 64, reflections=reflections, pos=pos, rot=rot, scale=scale)
        core, view = _core_for(host, reflections)
        try:
            pixels = np.arange(96 * 64, dtype=np.uint32)[::3]
            o, d, w = core.camera_rays(pixels, 5, 16)
            ro, rd, rw = _restated_rays(lib, _physical_camera(None, reflections, host.get_camera()), view.width, view.height, list(view.cam_pos),
                                        list(view.cam_rotation), view.cam_scale, pixels, 5, 16)
            assert np.array_equal(w.view(np.uint32), rw.view(np.uint32)), "weights (and so validity) bit for bit"
            assert np.array_equal(o.view(np.uint32), ro.view(np.uint32)) and np.array_equal(d.view(np.uint32), rd.view(np.uint32))
            assert 0.05 < (w > 0).mean() < 1.0, "some rays leave the lens, some do not"
            total += w.size
        finally:
            core.close()
            host.close()
    assert total >= 64 * 1024 // 2


@pytest.mark.gpu
def test_a_singlet_focuses_at_the_paraxial_object_distance():
    """A biconvex singlet through the ext API with a small exit pupil, the sensor at the float64 paraxial image distance of an object plane at 2 m: the
    exit rays of one pixel meet in a spot at 2 m that is at least 5x tighter (RMS) than at 1 m and 4 m."""
    R, T, nglass, D = 40.0, 6.0, 1.5, 2000.0
    # interface i: centre at vertex - radius; the first surface is convex towards the sensor, the second towards the scene
    g = {"interfaces": [[-R, 0.0, 15.0], [R, T, 15.0]], "media": [[1.0003, 0.0, FLT_MAX], [nglass, 60.0, 15.0], [1.0003, 0.0, FLT_MAX]]}
    n_air = float(np.float32(1.0003))

    def refr(n1, n2, rk):  # paraxial refraction, (height, angle); rk > 0: the centre lies beyond the surface along the light
        return np.array([[1, 0], [-(n2 - n1) / (n2 * rk), n1 / n2]])

    def prop(t):
        return np.array([[1, t], [0, 1]])
    # light from the object's axis point, D in front of the second surface, through surfaces 2 and 1 onto the sensor side
    M = prop(0) @ refr(nglass, n_air, -R) @ prop(T) @ refr(n_air, nglass, R) @ prop(D)
    s = -M[0, 1] / M[1, 1]  # image distance behind the first surface (height 0 again)
    host = _host(8, 8)
    try:
        lens = CameraLens()
        lens.num_interfaces = 2
        for i, (r, v, cy) in enumerate(g["interfaces"]):
            lens.interfaces[i].radius, lens.interfaces[i].vertex, lens.interfaces[i].cylindrical_radius = r, v, cy
        for i, (n, a, cy) in enumerate(g["media"]):
            lens.media[i].design_ior, lens.media[i].abbe, lens.media[i].cylindrical_radius = n, a, cy
        host.set_camera_lens(lens)
        c = host.get_camera()
        c.physical.image_plane_distance = s
        c.physical.exit_pupil_point = 0.0
        c.physical.exit_pupil_diameter = 2.0
        c.physical.aperture_diameter = 1000.0
        c.physical.aperture_point = -1000.0
        c.physical.sensor_width = 0.01  # a 2.5 um pixel: the jitter inside it stays small at D
        host.set_camera(c)
        core, view = _core_for(host, False, g)
        try:
            o, d, w = core.camera_rays(np.array([3 + 3 * 8], np.uint32), 0, 256)
        finally:
            core.close()
        ok = w > 0
        assert ok.sum() > 200
        o, d = o[ok].astype(np.float64) * 1000.0, d[ok].astype(np.float64)  # m -> mm (camera at the origin, unrotated: the scene looks along -z)

        def rms(dist):
            t = (-(T + dist) - o[:, 2]) / d[:, 2]
            p = o[:, :2] + d[:, :2] * t[:, None]
            return np.sqrt(np.mean(np.sum((p - p.mean(0)) ** 2, 1)))
        at, near, far = rms(D), rms(D / 2), rms(2 * D)
        print("spot RMS at D/2, D, 2D: %.4f %.4f %.4f mm (image distance %.4f mm)" % (near, at, far, s))
        assert at * 5 < near and at * 5 < far
    finally:
        host.close()


@pytest.mark.gpu
def test_orientation_matches_the_thin_lens():
    """An emitter left of and above the axis lands in the same quadrant of the image with the physical camera as with the thin lens. The lens images
    the scene inverted onto the sensor and the sensor coordinate runs the other way (sensor x = width - step * px, camera_physical.cuh:15-17), like the
    thin lens's: the picture is upright."""
    quads = {}
    for physical in (False, True):
        host = _host(32, 32, depth=1, sky=(0.0, 0.0, 0.0))
        try:
            em = host.add_material(scenes._material((0.0, 0.0, 0.0), emission=(5.0, 5.0, 5.0)))
            x0, x1, y0, y1, z = -3.0, -1.0, 1.0, 3.0, -10.0
            q = np.float32([[x0, y0, z], [x1, y0, z], [x1, y1, z], [x0, y0, z], [x1, y1, z], [x0, y1, z]])
            host.new_instance(host.add_mesh(q.reshape(-1), np.full(2, em, np.uint16)))
            c = host.get_camera()
            c.use_physical_camera = physical
            c.thin_lens.fov = 1.0
            host.set_camera(c)
            host.render_samples(0, 16)
            fm, _ = host.accumulators()
            img = fm[0].reshape(32, 32)
            ys, xs = np.nonzero(img > 0)
            assert xs.size > 0
            quads[physical] = (xs.mean() < 16, ys.mean() < 16)
        finally:
            host.close()
    assert quads[True] == quads[False]


@pytest.mark.gpu
@pytest.mark.parametrize("reflections", [False, True])
def test_sky_only_image_is_the_sum_of_the_ray_weights(tmp_path_factory, reflections):
    lib = _check_lib(tmp_path_factory)
    sky = (0.75, 0.5, 0.25)
    host = _host(W, H, depth=1, sky=sky, reflections=reflections)
    core, view = _core_for(host, reflections)
    S = 8
    try:
        core.set_pixels(None)
        core.reset_counters()
        core.render(0, S, samples_per_pass=4)
        fm, _ = core.accumulators()
        traced = core.counters()[CNT_TRACE]
    finally:
        core.close()
    pixels = np.arange(W * H, dtype=np.uint32)
    _, _, w = _restated_rays(lib, _physical_camera(None, reflections, host.get_camera()), view.width, view.height, list(view.cam_pos), list(view.cam_rotation),
                             view.cam_scale, pixels, 0, S)
    host.close()
    w = w.reshape(S, W * H)
    rt = oracle_lib.lib().oracle_record_roundtrip
    want = np.zeros((3, W * H), np.float32)
    C3 = np.float32(sky)
    packed = (C.c_uint32 * 2)()
    for s in range(S):
        for p in range(W * H):
            if w[s, p] > 0:
                inp, out = (C.c_float * 3)(w[s, p], w[s, p], w[s, p]), (C.c_float * 3)()
                rt(inp, packed, out)
                want[:, p] = want[:, p] + C3 * np.float32(list(out))
    assert np.array_equal(fm, want)
    assert traced == int((w > 0).sum()), "invalid rays are neither queued nor traced"


def _physical_frames(host_fn, mode):
    host = host_fn()
    try:
        if mode == "adaptive":
            s = host.get_settings()
            s.enable_adaptive_sampling = True
            s.adaptive_sampling_max_sampling_rate = 1
            s.adaptive_sampling_avg_sampling_rate = 1
            host.set_settings(s)
        if mode == "preview":
            s = host.get_settings()
            s.undersampling = 2
            host.set_settings(s)
            host.set_output_properties(s.width, s.height)
        host.render(3)
        return host.accumulators(), host.ray_counters()[:4]
    finally:
        host.close()


@pytest.mark.gpu
def test_adaptive_and_preview_passes_equal_the_uniform_render():
    """k_generate_adaptive<physical> at rate 1 and the undersampling preview (k_generate<physical> over a pixel list) start the same paths."""
    mk = lambda: _host(W, H, depth=3, plane_z=-4.0, reflections=True)
    (fm, sm), cnt = _physical_frames(mk, "uniform")
    for mode in ("adaptive", "preview"):
        (fm2, sm2), _ = _physical_frames(mk, mode)
        assert np.array_equal(fm, fm2) and np.array_equal(sm, sm2), mode
    assert float(fm.max()) > 0


@pytest.mark.gpu
def test_eight_device_slots_equal_one_device(tmp_path, monkeypatch):
    import test_multi_gpu
    test_multi_gpu._eight_slot_host_equals_one_device(lambda: _host(256, 128, depth=3, plane_z=-4.0), tmp_path, monkeypatch, 2)  # 32 tiles: every slot gets some


@pytest.mark.gpu
def test_purkinje_is_off_behind_the_physical_camera():
    imgs = {}
    for physical in (False, True):
        for purkinje in (False, True):
            host = _host(W, H, depth=1, sky=(0.00005, 0.0001, 0.0002))  # below the shift's luminance threshold (purkinje.cuh)
            try:
                c = host.get_camera()
                c.use_physical_camera = physical
                c.purkinje = purkinje
                c.exposure = 8.0  # applied after the shift (tonemap.cuh): the dim frame becomes visible
                host.set_camera(c)
                host.set_output_properties(W, H)
                host.render(2)
                imgs[physical, purkinje] = host.get_image(host.acquire_output())[0].copy()
            finally:
                host.close()
    assert np.array_equal(imgs[True, True], imgs[True, False])
    assert not np.array_equal(imgs[False, True], imgs[False, False]), "guard: the thin lens's shift shows"


@pytest.mark.gpu
def test_pixel_query_follows_the_physical_ray(tmp_path_factory):
    lib = _check_lib(tmp_path_factory)
    host = _host(W, H, plane_z=-5.0)
    core, view = _core_for(host)
    try:
        pixels = np.arange(W * H, dtype=np.uint32)
        o, d, w = _restated_rays(lib, _physical_camera(None, False, host.get_camera()), view.width, view.height, list(view.cam_pos),
                                 list(view.cam_rotation), view.cam_scale, pixels, 0, 1)
        valid_seen = invalid_seen = 0
        for p in range(0, W * H, 7):
            x, y = p % W, p // W
            inst, _, t, _ = core.pixel_query(x, y)
            if w[p] > 0:
                hit = (-5.0 - o[p, 2]) / d[p, 2]
                px_, py_ = o[p, 0] + d[p, 0] * hit, o[p, 1] + d[p, 1] * hit
                want = 0 if (hit > 0 and abs(px_) < 20 and abs(py_) < 20) else 0xFFFFFFFE
                assert inst == want
                valid_seen += 1
            else:
                assert inst == 0xFFFFFFFF and t == FLT_MAX
                invalid_seen += 1
        assert valid_seen > 0 and invalid_seen > 0
    finally:
        core.close()
        host.close()


@pytest.mark.gpu
def test_fast_flavour_rays_are_close_to_exact():
    host = _host(96, 64, reflections=False)
    core, view = _core_for(host)
    try:
        pixels = np.arange(96 * 64, dtype=np.uint32)
        o, d, w = core.camera_rays(pixels, 0, 11)
        core.set_flavour("fast")
        fo, fd, fw = core.camera_rays(pixels, 0, 11)
    finally:
        core.close()
        host.close()
    assert np.mean((w > 0) != (fw > 0)) <= 0.001
    both = (w > 0) & (fw > 0)
    rel = lambda a, b: np.linalg.norm(a - b, axis=1) / np.linalg.norm(b, axis=1)
    print("fast vs exact: validity differs on %.4f %% of the rays; origins %.2e, directions %.2e relative" % (
        100 * np.mean((w > 0) != (fw > 0)), rel(fo[both], o[both]).max(), rel(fd[both], d[both]).max()))
    assert rel(fo[both], o[both]).max() < 2e-5 and rel(fd[both], d[both]).max() < 2e-5
