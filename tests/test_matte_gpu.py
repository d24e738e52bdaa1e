"""ID mattes on the device (include/lum_core.h lumc_render_first_hits / lumc_download_mattes / lumc_matte_mask; csrc/host/matte.hip; include/luminary_amd.h
luminary_ext_render_mattes).

The kernels are held to the host twin (lumc_matte_host, which tests/test_matte.py holds to a restatement of the definition) byte for byte. The id streams the twin
is fed come by a route that shares nothing with the first-hit passes but the camera and the scene: every camera ray of the frame (lumc_camera_rays), its closest
hit through the ray query (lumc_trace_closest_host), and the material from the view's own arrays as luminary_host_get_pixel_info derives it."""
import ctypes as C

import numpy as np
import pytest

import luminary_amd
import oracle_lib
from luminary_amd import Vec3, scenes
from luminary_amd.core import (DIRTY_INSTANCE_TRANSFORMS, DIRTY_LIGHTS, FIRST_HIT_GUIDES, FIRST_HIT_MATTES, MATTE_ID_EMPTY as EMPTY, MATTE_ID_MISS, MATTE_ID_OCEAN,
                               MATTE_INSTANCE, MATTE_MATERIAL, Core, CoreError, matte_host, matte_mask_host_twin)

pytestmark = pytest.mark.gpu
F, U = np.float32, np.uint32
LAYERS = {"instance": MATTE_INSTANCE, "material": MATTE_MATERIAL}


def _arr(ptr, count, dtype):
    return np.frombuffer(C.string_at(ptr, count * np.dtype(dtype).itemsize), dtype=dtype).copy()


def expected_ids(core, view, samples):
    """{layer: ids [samples, pixels]} by the independent route; EMPTY where the camera made no ray."""
    P = view.width * view.height
    o, d, weight = core.camera_rays(np.arange(P, dtype=U), 0, samples)
    hits = core.trace_closest_host(o, d, np.full((samples * P, 2), 0xFFFFFFFF, dtype=U))
    inst, tri = hits[:, 0], hits[:, 1]
    on_triangle = inst <= 0x7FFFFFFF
    offsets = _arr(view.mesh_tri_offset, view.num_meshes + 1, U)
    mesh_ids = _arr(view.instance_mesh_ids, view.num_instances, U)
    tri_tex = _arr(view.tri_tex, 4 * int(offsets[-1]), U).reshape(-1, 4)
    instance = np.where(on_triangle, inst, U(MATTE_ID_MISS)).astype(U)
    material = np.full(samples * P, MATTE_ID_MISS, U)
    material[on_triangle] = tri_tex[offsets[mesh_ids[inst[on_triangle]]].astype(np.int64) + tri[on_triangle], 3] & 0xFFFF
    for a in (instance, material):
        a[weight == 0] = EMPTY
    return {"instance": instance.reshape(samples, P), "material": material.reshape(samples, P)}, (weight != 0).reshape(samples, P)


def assert_tables(core, layer, want, where):
    """the raw slots and the ranks at R = 1, 6, 8 of a rendered layer against a twin's result, byte for byte"""
    si, sc, dropped = core.matte_tables(layer)
    for got, key in ((si, "slots_id"), (sc, "slots_count"), (dropped, "dropped")):
        bad = np.nonzero((got != want[key]).reshape(-1, got.shape[-1]).any(axis=0))[0]
        assert not bad.size, "%s: %s differs at %d pixels, first %s" % (where, key, bad.size, bad[:8])
    for ranks in (1, 6, 8):
        ids, cov, dr, rays = core.mattes(layer, ranks)
        assert np.array_equal(ids, want["ids"][:ranks]) and np.array_equal(cov.view(U), want["coverage"][:ranks].view(U)), (where, ranks)
        assert np.array_equal(dr, want["dropped"]) and np.array_equal(rays, want["rays"]), (where, ranks)


def _zoo_core(width=50, height=31, flavour="exact"):
    host = scenes.zoo_scene(width, height, bounces=2)
    view = oracle_lib.with_luts(host.device_scene())
    core = Core(0)
    core.set_flavour(flavour)
    core.upload(view)
    return host, view, core


@pytest.mark.parametrize("samples", [1, 5, 16])
def test_tables_and_ranks_equal_the_twin(samples):
    """50 x 31: seven workgroups of 256 with a part-empty last wave. Several instances meet in many pixels: ranking and ties."""
    host, view, core = _zoo_core()
    try:
        core.render_first_hits(samples, FIRST_HIT_MATTES, MATTE_INSTANCE | MATTE_MATERIAL)
        assert core.has_mattes() and not core.has_guides()
        want, _ = expected_ids(core, view, samples)
        for name, layer in LAYERS.items():
            twin = matte_host(want[name], 8)
            assert_tables(core, layer, twin, "%s, %d samples" % (name, samples))
            assert not twin["dropped"].any() and (twin["rays"] == samples).all()
            if samples > 1 and name == "instance":
                assert ((twin["slots_count"] > 0).sum(axis=0) > 1).sum() > 50, "edges: pixels that saw more than one id"
        st = core.matte_stats()
        assert (st.samples, st.layers, st.bytes, st.valid, list(st.dropped_pixels)) == (samples, 3, 136 * 50 * 31, 1, [0, 0]) and st.seconds > 0.0
    finally:
        core.close()
        host.close()


def test_a_pixel_that_sees_more_than_eight_instances_drops_the_rest():
    """The benchmark scene at 12 x 8: a pixel is a large part of the frame, and 64 sample ids find up to thirteen instances in one."""
    host = scenes.example_scene(12, 8, bounces=2)
    view = oracle_lib.with_luts(host.device_scene())
    core = Core(0)
    try:
        core.set_flavour("exact")
        core.upload(view)
        core.render_first_hits(64, FIRST_HIT_MATTES, MATTE_INSTANCE)
        want, _ = expected_ids(core, view, 64)
        twin = matte_host(want["instance"], 8)
        print("pixels with dropped samples: %d, samples dropped: %d" % (int((twin["dropped"] > 0).sum()), int(twin["dropped"].sum())))
        assert (twin["dropped"] > 0).any(), "the case must overflow the eight slots, or it shows nothing"
        assert_tables(core, MATTE_INSTANCE, twin, "overflow")
        st = core.matte_stats()
        assert list(st.dropped_pixels) == [int((twin["dropped"] > 0).sum()), 0] and st.layers == MATTE_INSTANCE and st.bytes == 68 * 96
        with pytest.raises(CoreError, match="did not ask for this layer"):
            core.mattes(MATTE_MATERIAL, 8)
    finally:
        core.close()
        host.close()


def test_guides_and_mattes_from_one_trace_are_those_of_two():
    host, view, core = _zoo_core()
    try:
        guides = [g.copy() for g in core.render_guides(5)]
        core.render_first_hits(5, FIRST_HIT_MATTES, 3)
        alone = {layer: core.matte_tables(layer) + core.mattes(layer, 8) for layer in LAYERS.values()}
        # lumc_render_guides on a context that holds mattes leaves them alone
        core.render_guides(3)
        assert core.has_mattes()
        for layer in LAYERS.values():
            for a, b in zip(alone[layer], core.matte_tables(layer) + core.mattes(layer, 8)):
                assert np.array_equal(a.view(U), b.view(U))
        core.matte_release()
        assert not core.has_mattes() and core.matte_stats().bytes == 0
        with pytest.raises(CoreError, match="no mattes"):
            core.mattes(MATTE_INSTANCE, 8)
        core.render_first_hits(5, FIRST_HIT_GUIDES | FIRST_HIT_MATTES, 3)
        assert core.has_mattes() and core.has_guides()
        for a, b in zip(guides, core.guides()):
            assert np.array_equal(a.view(U), b.view(U)), "the guide planes of lumc_render_guides, bit for bit"
        for layer in LAYERS.values():
            for a, b in zip(alone[layer], core.matte_tables(layer) + core.mattes(layer, 8)):
                assert np.array_equal(a.view(U), b.view(U)), "the mattes of MATTES alone, byte for byte"
        for bad in ((5, 0, 3), (5, 4, 3), (5, FIRST_HIT_MATTES, 0), (5, FIRST_HIT_MATTES, 4), (1025, FIRST_HIT_MATTES, 3)):
            with pytest.raises(CoreError):
                core.render_first_hits(*bad)
        for ranks in (0, 9):
            with pytest.raises(CoreError, match="ranks"):
                core.mattes(MATTE_INSTANCE, ranks)
        with pytest.raises(CoreError, match="layer"):
            core.mattes(3, 8)
        with pytest.raises(CoreError, match="at most 16"):
            core.matte_mask(MATTE_INSTANCE, np.arange(17))
    finally:
        core.close()
        host.close()


def test_one_layer_alone_holds_what_both_hold():
    host, view, core = _zoo_core()
    try:
        core.render_first_hits(5, FIRST_HIT_MATTES, 3)
        both = {layer: core.matte_tables(layer) for layer in LAYERS.values()}
        for layer in LAYERS.values():
            core.render_first_hits(5, FIRST_HIT_MATTES, layer)
            st = core.matte_stats()
            assert (st.layers, st.bytes) == (layer, 68 * 50 * 31), "one layer allocates half"
            for a, b in zip(both[layer], core.matte_tables(layer)):
                assert np.array_equal(a, b)
            with pytest.raises(CoreError, match="did not ask for this layer"):
                core.matte_tables(layer ^ 3)
    finally:
        core.close()
        host.close()


def test_samples_without_a_path_count_nowhere():
    """Behind a physical camera some rays do not leave the lens: they are in no slot, not in dropped and not in rays."""
    import test_physical_camera as tpc
    host = scenes.zoo_scene(50, 31, bounces=2)
    c = host.get_camera()
    c.use_physical_camera = True
    host.set_camera(c)
    core, view = tpc._core_for(host)
    try:
        core.render_first_hits(5, FIRST_HIT_MATTES, 3)
        want, has_path = expected_ids(core, view, 5)
        assert 0 < (~has_path).sum() < has_path.size, "some rays, not all, end in the lens"
        for name, layer in LAYERS.items():
            assert_tables(core, layer, matte_host(want[name], 8), name + " behind a lens")
            _, cov, dropped, rays = core.mattes(layer, 8)
            assert np.array_equal(rays, has_path.sum(axis=0)) and not dropped.any()
            # counts / 5 add up exactly in float64; a coverage is the float32 nearest to its count / 5
            assert np.array_equal(np.rint(cov.astype(np.float64) * 5).sum(axis=0), rays)
    finally:
        core.close()
        host.close()


def test_open_water_is_the_ocean_in_both_layers():
    """No geometry, the camera above the water and looking down at it: the lower part of the frame ends on the surface, the upper part in the sky."""
    host = scenes.edge_scene("empty", 48, 32, 2)
    scenes.set_camera(host, (0.0, 3.0, 0.0), (-0.4, 0.0, 0.0))
    o = host.get_ocean()
    o.active, o.height, o.amplitude = True, 0.0, 0.5
    host.set_ocean(o)
    view = oracle_lib.with_luts(host.device_scene())
    core = Core(0)
    try:
        core.set_flavour("exact")
        core.upload(view)
        _, _, depth = core.render_guides(1)
        on_water = (depth != -1.0).reshape(-1)  # sample id 0: with no geometry every hit is the surface
        assert 100 < on_water.sum() < on_water.size - 100
        core.render_first_hits(1, FIRST_HIT_MATTES, 3)
        for layer in LAYERS.values():
            ids, cov, _, _ = core.mattes(layer, 2)
            assert np.array_equal(ids[0], np.where(on_water, U(MATTE_ID_OCEAN), U(MATTE_ID_MISS))) and (cov[0] == 1.0).all() and (ids[1] == EMPTY).all()
        core.render_first_hits(5, FIRST_HIT_MATTES, 3)
        for layer in LAYERS.values():
            si, sc, dropped = core.matte_tables(layer)
            ids, cov, _, rays = core.mattes(layer, 8)
            assert np.array_equal(sc.sum(axis=0) + dropped, rays) and (rays == 5).all() and not dropped.any()
            assert set(np.unique(ids).tolist()) == {MATTE_ID_OCEAN, MATTE_ID_MISS, EMPTY}
            all_water = (si[0] == MATTE_ID_OCEAN) & (sc[0] == 5)
            assert all_water.sum() > 100 and (ids[0][all_water] == MATTE_ID_OCEAN).all() and (cov[0][all_water].view(U) == F(1.0).view(U)).all()
            no_water = ~(si == MATTE_ID_OCEAN).any(axis=0)
            assert all_water.reshape(32, 48)[-1].all(), "water at the lower edge of the frame"
            assert no_water.any() and (ids[0][no_water] == MATTE_ID_MISS).all() and (cov[0][no_water] == 1.0).all(), "sky where no sample met the water"
    finally:
        core.close()
        host.close()


def test_the_fast_flavour_keeps_the_invariants():
    """No equality with the exact flavour is asked: a last-bit difference of a ray may move an edge sample. The tables obey the definition."""
    host, view, core = _zoo_core(flavour="fast")
    try:
        assert core.flavour == "fast"
        core.render_first_hits(16, FIRST_HIT_MATTES, 3)
        for layer in LAYERS.values():
            si, sc, dropped = core.matte_tables(layer)
            ids, cov, dr, rays = core.mattes(layer, 8)
            assert np.array_equal(sc.sum(axis=0) + dropped, rays) and (rays == 16).all() and np.array_equal(dr, dropped)
            counts = np.rint(cov.astype(np.float64) * 16).astype(np.int64)
            assert (np.diff(counts, axis=0) <= 0).all(), "ranks in non-increasing count"
            tie = (np.diff(counts, axis=0) == 0) & (counts[1:] > 0)
            assert (ids[1:][tie] > ids[:-1][tie]).all(), "ties in ascending id"
            # the ranks are what the twin makes of the device's own slots: each slot's id as often as its count, slot after slot
            stream = np.full((16, si.shape[1]), EMPTY, U)
            at = np.zeros(si.shape[1], np.int64)
            for k in range(8):
                for p in np.nonzero(sc[k])[0]:
                    stream[at[p]:at[p] + sc[k, p], p] = si[k, p]
                    at[p] += sc[k, p]
            twin = matte_host(stream, 8)
            assert np.array_equal(twin["slots_id"], si) and np.array_equal(twin["slots_count"], sc)
            assert np.array_equal(twin["ids"], ids) and np.array_equal(twin["coverage"].view(U), cov.view(U))
    finally:
        core.close()
        host.close()


def test_the_mask_equals_its_twin():
    host, view, core = _zoo_core()
    try:
        core.render_first_hits(16, FIRST_HIT_MATTES, 3)
        for layer in LAYERS.values():
            si, sc, dropped = core.matte_tables(layer)
            _, _, _, rays = core.mattes(layer, 1)
            present = np.unique(si[sc > 0])
            for want in ([], present[:1], present[:16], [12345678], [EMPTY], list(present[:3]) + [int(present[0])]):
                got = core.matte_mask(layer, want)
                assert np.array_equal(got.view(U), matte_mask_host_twin(si, sc, 16, want).view(U)), (layer, want)
            if present.size <= 16:  # every id of the frame: all that the tables hold
                everything = core.matte_mask(layer, present)
                assert np.array_equal((everything.astype(np.float64) * 16 + dropped), rays.astype(np.float64))
            busiest = int(np.argmax((sc > 0).sum(axis=0)))
            own = core.matte_mask(layer, si[:, busiest])
            assert own[busiest] * 16 + dropped[busiest] == rays[busiest], "a pixel's own ids and what it dropped are all its samples"
    finally:
        core.close()
        host.close()


def test_scene_and_lens_changes_make_the_mattes_stale():
    import test_physical_camera as tpc
    host, view, core = _zoo_core()
    try:
        core.render_first_hits(5, FIRST_HIT_MATTES, 3)
        ids, _, _, _ = core.mattes(MATTE_INSTANCE, 1)
        first = ids[0]
        seen = [int(i) for i in np.unique(first) if i < host.get_num_instances() and 20 < (first == i).sum() < 400]
        assert seen, "an instance that is the first id of a part of the frame"
        moved_id = seen[0]
        inst = host.get_instance(moved_id)
        inst.position = Vec3(inst.position.x + 0.4, inst.position.y + 0.3, inst.position.z)
        host.set_instance_transforms([inst])
        view = oracle_lib.with_luts(host.device_scene())
        core.update(view, DIRTY_INSTANCE_TRANSFORMS | DIRTY_LIGHTS)
        assert not core.has_mattes()
        with pytest.raises(CoreError, match="stale: the scene was uploaded or updated"):
            core.mattes(MATTE_INSTANCE, 1)
        with pytest.raises(CoreError, match="stale"):
            core.matte_mask(MATTE_INSTANCE, [moved_id])
        core.render_first_hits(5, FIRST_HIT_MATTES, 3)
        want, _ = expected_ids(core, view, 5)
        assert_tables(core, MATTE_INSTANCE, matte_host(want["instance"], 8), "after the move")
        after = core.mattes(MATTE_INSTANCE, 1)[0][0]
        new = (after == moved_id) & (first != moved_id)
        assert new.any() and ((first == moved_id) & (after != moved_id)).any(), "the moved instance ranks first at pixels it did not cover, and left others"
        core.set_physical_camera(tpc._physical_camera(None, False, host.get_camera()))
        with pytest.raises(CoreError, match="stale: the camera's lens was set"):
            core.mattes(MATTE_INSTANCE, 1)
        core.render_first_hits(5, FIRST_HIT_MATTES, MATTE_INSTANCE)
        assert core.has_mattes() and core.mattes(MATTE_INSTANCE, 1)[0].shape == (1, 50 * 31)
    finally:
        core.close()
        host.close()


def test_the_public_api_equals_the_core():
    w, h = 50, 31
    host = scenes.zoo_scene(w, h, bounces=2)
    core = Core(0)
    try:
        lib = luminary_amd._lib()
        host.set_denoiser(enabled=True, guide_samples=5)
        host.render_mattes(5)
        ctx = C.c_void_p(host.core_context())
        assert lib.lumc_has_guides(ctx) == 1 and lib.lumc_has_mattes(ctx) == 1, "the denoiser's guides come from the same rays"
        core.set_flavour("exact")
        core.upload(oracle_lib.with_luts(host.device_scene()))
        core.render_first_hits(5, FIRST_HIT_GUIDES | FIRST_HIT_MATTES, 3)
        for layer in (luminary_amd.MATTE_LAYER_INSTANCE, luminary_amd.MATTE_LAYER_MATERIAL):
            ids, cov = host.matte(layer, 6, w, h)
            want_ids, want_cov, _, _ = core.mattes(layer, 6)
            assert np.array_equal(ids.reshape(6, -1), want_ids) and np.array_equal(cov.reshape(6, -1).view(U), want_cov.view(U))
            some = np.unique(want_ids[0])[:3]
            assert np.array_equal(host.matte_mask(layer, some, w, h).reshape(-1).view(U), core.matte_mask(layer, some).view(U))
        for a, b in zip(host.first_hit_guides(w, h), core.guides()):
            assert np.array_equal(a.view(U), b.view(U))
        st = host.matte_stats()
        assert (st["renders"], st["valid"], st["samples"], st["layers"], st["bytes"], st["dropped_pixels"]) == (1, 1, 5, 3, 136 * w * h, [0, 0])
        for args in ((luminary_amd.MATTE_LAYER_INSTANCE, 6, w + 1, h), (luminary_amd.MATTE_LAYER_INSTANCE, 9, w, h), (3, 6, w, h)):
            with pytest.raises(luminary_amd.LuminaryError) as e:
                host.matte(*args)
            assert e.value.code == 3, args
        with pytest.raises(luminary_amd.LuminaryError) as e:
            host.matte_mask(luminary_amd.MATTE_LAYER_INSTANCE, np.arange(17), w, h)
        assert e.value.code == 3
        # an edit of the scene: the getters refuse until the mattes are rendered again
        inst = host.get_instance(0)
        inst.position = Vec3(inst.position.x + 0.25, inst.position.y, inst.position.z)
        host.set_instance(inst)
        with pytest.raises(luminary_amd.LuminaryError) as e:
            host.matte(luminary_amd.MATTE_LAYER_INSTANCE, 6, w, h)
        assert e.value.code == 7 and host.matte_stats()["valid"] == 0
        host.render_mattes(5, luminary_amd.MATTE_LAYER_INSTANCE)
        assert host.matte(luminary_amd.MATTE_LAYER_INSTANCE, 1, w, h)[0].shape == (1, h, w) and host.matte_stats()["renders"] == 2
    finally:
        core.close()
        host.close()
