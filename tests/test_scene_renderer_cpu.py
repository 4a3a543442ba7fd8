"""CPU: the multi-object scene renderer (Panda3dSceneRenderer / mp_raster_render_scene) without a GPU -- its host rules (scene radius,
light rig, TCO), its error cases, its API shape against the reference, and the host emulation of the scene tile kernel
(tests/raster_scene_emul.cpp: the device code's raster_scene_core.h in the kernel's order) against the independent oracle
(oracle/raster.c), bit for bit."""
import dataclasses
import inspect

import numpy as np
import pytest

K_FULL = np.array([[605.95, 0, 319.03], [0, 605.0, 249.68], [0, 0, 1]], np.float32)
K_HALF = np.array([[302.9, 0, 160.2], [0, 302.5, 119.7], [0, 0, 1]], np.float32)   # 320 x 240
K_TINY = np.array([[80.5, 0, 40.1], [0, 80.2, 29.8], [0, 0, 1]], np.float32)       # 80 x 60


def _rot(rng):
    q = rng.randn(4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _pose(rng, t_scale=1.0):
    T = np.eye(4)
    T[:3, :3] = _rot(rng)
    T[:3, 3] = rng.randn(3) * t_scale
    return T


def _poses(n, seed, z=(0.35, 0.7), xy=0.12):
    from tests.support import synthetic as syn

    rng = np.random.RandomState(seed)
    return np.stack([syn.random_pose(rng, z_range=z, xy_frac=xy) for _ in range(n)])


# ---------------------------------------------------------------------------------------------------------- host rules
def test_scene_radius_of_one_object_is_the_mesh_radius_bit_for_bit(engine_meshes):
    from megapose6d_amd.scene_renderer import aabb_centre, scene_sphere
    from oracle import raster as orr

    rng = np.random.RandomState(0)
    for m in engine_meshes:
        r = orr.mesh_radius(m["vertices"])   # the float32 rule of mp_mesh_db_radius, restated by the oracle
        c = aabb_centre(m["vertices"]).astype(np.float64)
        for _ in range(5):
            T = _pose(rng, 3.0)
            _, rs = scene_sphere([T[:3, :3] @ c + T[:3, 3]], [r])
            assert np.float32(rs) == np.float32(r)


def test_sphere_fold_encloses_both_and_is_tight_when_one_contains_the_other():
    from megapose6d_amd.scene_renderer import enclose_spheres, scene_sphere

    rng = np.random.RandomState(1)
    for _ in range(200):
        c1, c2 = rng.randn(3), rng.randn(3)
        r1, r2 = rng.rand() * 2, rng.rand() * 2
        c, r = enclose_spheres(c1, r1, c2, r2)
        for ci, ri in ((c1, r1), (c2, r2)):
            assert np.linalg.norm(ci - c) + ri <= r * (1 + 1e-12) + 1e-12
        d = np.linalg.norm(c2 - c1)
        if d + r2 <= r1:
            assert r == r1 and np.array_equal(c, c1)
        elif d + r1 <= r2:
            assert r == r2 and np.array_equal(c, c2)
        else:
            assert abs(r - 0.5 * (d + r1 + r2)) < 1e-12   # no enclosing sphere is smaller
    c, r = enclose_spheres(np.zeros(3), 1.0, np.array([0.1, 0, 0]), 0.5)   # contained: the big sphere itself
    assert r == 1.0 and np.array_equal(c, np.zeros(3))
    c, r = enclose_spheres(np.array([0.1, 0, 0]), 0.5, np.zeros(3), 1.0)
    assert r == 1.0 and np.array_equal(c, np.zeros(3))
    c, r = scene_sphere([np.zeros(3), np.array([0.1, 0, 0]), np.array([2.0, 0, 0])], [1.0, 0.5, 1.0])
    assert abs(r - 2.0) < 1e-12 and np.allclose(c, [1.0, 0, 0])
    assert scene_sphere([], [])[1] == 0.0


def test_light_rig_at_identity_is_the_batch_renderers_and_places_lights_in_the_world():
    from megapose6d_amd import engine as eng
    from megapose6d_amd.renderer import _to_engine_lights
    from megapose6d_amd.scene_renderer import object_light_rig, parse_scene_lights
    from megapose6d_amd.types import Panda3dLightData, make_scene_lights

    lights = make_scene_lights() + [Panda3dLightData("point", (0.2, 0.1, 0.3, 1.0), positioning_function=lambda root, node: node.setPos(
        0.3 * root.getBounds().radius + 0.05, -0.02, 0.5))]
    amb, cols, dirs, offs = parse_scene_lights(lights)
    ref = _to_engine_lights(lights)   # what Panda3dBatchRenderer passes (renderer.py:21-65)
    d_o, o_o = object_light_rig(dirs, offs, np.eye(4))
    got = eng.make_lights(tuple(amb), [tuple(v) for v in d_o], cols, [tuple(v) for v in o_o])
    assert bytes(got) == bytes(ref)
    rng = np.random.RandomState(2)
    for _ in range(10):
        TWO = _pose(rng, 0.5)
        radius = rng.rand() * 0.2 + 0.01
        d_o, o_o = object_light_rig(dirs, offs, TWO)
        d_o, o_o = d_o.astype(np.float32).astype(np.float64), o_o.astype(np.float32).astype(np.float64)   # what the engine receives
        p_world = (d_o * 10 * radius + o_o) @ TWO[:3, :3].T + TWO[:3, 3]
        assert np.abs(p_world - (dirs * 10 * radius + offs)).max() < 1e-6


def test_tco_composition():
    from megapose6d_amd.scene_renderer import scene_tco

    rng = np.random.RandomState(3)
    TWC, TWO = _pose(rng), _pose(rng)
    T = scene_tco(TWC, TWO)
    assert np.allclose(TWC @ T, TWO, atol=1e-12)
    assert np.array_equal(scene_tco(np.eye(4), TWO), TWO)
    p = np.array([0.1, 0.2, 0.3, 1.0])
    assert np.allclose(T @ p, np.linalg.inv(TWC) @ (TWO @ p), atol=1e-12)


# ---------------------------------------------------------------------------------------------------------- errors (raised before any GPU work)
@pytest.fixture()
def scene_renderer(object_dataset):
    from megapose6d_amd.scene_renderer import Panda3dSceneRenderer

    return Panda3dSceneRenderer(object_dataset)


def _cam(**kw):
    from megapose6d_amd.types import Panda3dCameraData

    return Panda3dCameraData(K=K_FULL.astype(np.float64), resolution=(48, 64), **kw)


def test_errors_for_what_the_contract_does_not_render(scene_renderer, object_dataset):
    from megapose6d_amd.types import Panda3dLightData, Panda3dObjectData, make_scene_lights

    lab = object_dataset.list_objects[0].label
    L = make_scene_lights()
    cases = [
        ([Panda3dObjectData(lab, color=(1.0, 0.0, 0.0, 1.0))], [_cam()], L),
        ([Panda3dObjectData(lab, material=object())], [_cam()], L),
        ([Panda3dObjectData(lab, scale=2.0)], [_cam()], L),
        ([Panda3dObjectData(lab, positioning_function=lambda r, n: None)], [_cam()], L),
        ([Panda3dObjectData(lab)], [_cam(positioning_function=lambda r, n: None)], L),
        ([Panda3dObjectData(lab)], [_cam(z_near=0.01)], L),
        ([Panda3dObjectData(lab)], [_cam(z_far=100)], L),
        ([Panda3dObjectData(lab)], [_cam()], [Panda3dLightData("directional", positioning_function=lambda r, n: n.setPos(0, 0, 1))]),
        ([Panda3dObjectData(lab)], [_cam()], make_scene_lights() + make_scene_lights()[1:4]),   # 9 point lights
    ]
    for objs, cams, lights in cases:
        with pytest.raises(NotImplementedError):
            scene_renderer.render_scene(objs, cams, lights)
    with pytest.raises(KeyError):
        scene_renderer.render_scene([Panda3dObjectData("no_such_label")], [_cam()], L)
    with pytest.raises(AssertionError):
        scene_renderer.render_scene([Panda3dObjectData(lab)], [_cam()], L, render_binary_mask=True)
    with pytest.raises(KeyError):
        type(scene_renderer)(object_dataset, preload_labels={"no_such_label"})
    with pytest.raises(ValueError):
        type(scene_renderer)(object_dataset, msaa=2)


def test_transform_objects_and_remove_mesh_material_are_accepted():
    from megapose6d_amd.types import Panda3dObjectData, pose_matrix

    class Transform:   # the reference's lib3d Transform: anything with toHomogeneousMatrix()
        def __init__(self, M):
            self.M = M

        def toHomogeneousMatrix(self):
            return self.M

    M = _pose(np.random.RandomState(4))
    assert np.array_equal(pose_matrix(Transform(M)), M)
    assert np.array_equal(pose_matrix(M.tolist()), M)
    assert np.array_equal(pose_matrix(Panda3dObjectData("x").TWO), np.eye(4))
    assert Panda3dObjectData("x", remove_mesh_material=True).remove_mesh_material   # accepted and ignored (the contract has no materials)
    with pytest.raises(ValueError):
        pose_matrix(np.eye(3))


# ---------------------------------------------------------------------------------------------------------- API shape
def _params(fn):
    return [(p.name, p.default) for p in inspect.signature(fn).parameters.values() if p.name != "self"]


def _fields(cls):
    return [(f.name, f.default) for f in dataclasses.fields(cls)]


def test_api_shape_matches_the_reference():
    from megapose6d_amd import CameraRenderingData, Panda3dCameraData, Panda3dObjectData, Panda3dSceneRenderer
    from megapose6d_amd.types import pose_matrix

    E, M = inspect.Parameter.empty, dataclasses.MISSING
    # panda3d_scene_renderer.py:145-151 (+ the engine's trailing msaa keyword)
    assert _params(Panda3dSceneRenderer.__init__) == [("asset_dataset", E), ("preload_labels", set()), ("debug", False), ("verbose", False),
                                                      ("msaa", 4)]
    # panda3d_scene_renderer.py:298-308
    assert _params(Panda3dSceneRenderer.render_scene) == [("object_datas", E), ("camera_datas", E), ("light_datas", E), ("render_depth", False),
                                                          ("copy_arrays", True), ("render_binary_mask", False), ("render_normals", False),
                                                          ("clear", True)]
    # panda3d_renderer/types.py:43-55
    assert _fields(CameraRenderingData) == [("rgb", M), ("normals", None), ("depth", None), ("binary_mask", None)]
    # panda3d_renderer/types.py:58-66 (TWC default: the identity Transform)
    f = _fields(Panda3dCameraData)
    assert [n for n, _ in f] == ["K", "resolution", "TWC", "z_near", "z_far", "node_name", "positioning_function"]
    assert [d for _, d in f[:2]] == [M, M] and [d for _, d in f[3:]] == [0.1, 10, "camera", None]
    assert np.array_equal(pose_matrix(f[2][1]), np.eye(4))
    # panda3d_renderer/types.py:117-125 (TWO default: the identity Transform)
    f = _fields(Panda3dObjectData)
    assert [n for n, _ in f] == ["label", "TWO", "color", "material", "remove_mesh_material", "scale", "positioning_function"]
    assert f[0][1] is M and [d for _, d in f[2:]] == [None, None, False, 1, None]
    assert np.array_equal(pose_matrix(f[1][1]), np.eye(4))


# ---------------------------------------------------------------------------------------------------------- emulation vs oracle
def _oracle_rig(positions, colors, ambient=(0.1, 0.1, 0.1)):
    """object-frame point lights given as positions: dir = 0, offset = position (no radius enters)"""
    from oracle import raster as orr

    return orr.lights_struct(ambient, [(0.0, 0.0, 0.0)] * len(positions), colors, positions)


def _axis_rig():
    from oracle import raster as orr

    return orr.lights_struct((0.1, 0.1, 0.1), orr.POINT_DIRS, [(0.4, 0.4, 0.4)] * 6)


def _one_object(mesh, T, K, h, w, flags, L, **kw):
    """one object per camera: the emulation with the mesh radius as scene radius == oracle.raster.render"""
    from oracle import raster as orr
    from tests.support import raster_scene as rsc

    r = orr.mesh_radius(mesh["vertices"])
    n = T.shape[0]
    rgb_o, nrm_o, dep_o = orr.render(mesh, T, K, h, w, flags, L)
    rgb_e, nrm_e, dep_e, inst = rsc.render([mesh], list(range(n + 1)), [0] * n, T, K, [r] * n, [L] * n, h, w, flags, **kw)
    assert np.array_equal(rgb_e, rgb_o), ("rgb", (rgb_e != rgb_o).mean())
    if flags & 1:
        assert np.array_equal(nrm_e, nrm_o), ("normals", (nrm_e != nrm_o).mean())
    if flags & 2:
        assert np.array_equal(dep_e, dep_o), ("depth", np.abs(dep_e - dep_o).max())
        assert np.array_equal(inst, np.where(dep_o > 0, 0, -1))
    return rgb_o, dep_o


@pytest.mark.parametrize("msaa", [1, 4])
def test_one_object_scenes_equal_the_oracle(engine_meshes, msaa):
    T = _poses(2, 11)
    K = np.repeat(K_FULL[None], 2, 0)
    flags = 3 | (16 if msaa == 4 else 0)
    rgb, dep = _one_object(engine_meshes[0], T, K, 240, 320, flags, _axis_rig())
    assert (dep > 0).mean() > 0.02 and rgb.max() > 0.3
    _one_object(engine_meshes[1], T[:1], K[:1], 240, 320, flags | 4, _axis_rig(), reverse=1)   # GL eye normals, reversed lists


def test_one_object_scenes_textured_clipped_large_and_overflow(engine_meshes, tmp_path):
    from megapose6d_amd import mesh_io
    from tests.support import synthetic as syn

    tex = mesh_io.load_rigid_object(syn.make_textured_object(tmp_path, fmt="obj"))
    K = K_FULL[None]
    for msaa in (0, 16):
        _one_object(tex, _poses(1, 7, z=(0.3, 0.35), xy=0.02), K, 240, 320, 3 | msaa, _axis_rig())                  # texture
        _, dep = _one_object(engine_meshes[0], _poses(1, 3, z=(0.07, 0.11), xy=0.05), K, 240, 320, 3 | msaa, _axis_rig())   # near plane
        assert (dep > 0).mean() > 0.3
    v = np.array([[x, y, z] for x in (-0.1, 0.1) for y in (-0.07, 0.07) for z in (-0.05, 0.05)], np.float32)
    f = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]],
                 np.int32)
    box = dict(vertices=v, normals=(v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32),
               colors=((v - v.min(0)) / (v.max(0) - v.min(0))).astype(np.float32), faces=f)
    _one_object(box, _poses(1, 5, z=(0.3, 0.45), xy=0.05), K, 240, 320, 16 | 3, _axis_rig())                        # large pieces
    _one_object(engine_meshes[2], _poses(1, 6, z=(0.4, 0.5), xy=0.02), K, 120, 160, 16 | 3, _axis_rig(), cap_list=1)   # list overflow


def _composite(singles):
    """per-pixel nearest of single-object renders (rgb, nrm, dep) in list order; exactly equal depth -> the first object"""
    rgb = np.zeros_like(singles[0][0])
    nrm = np.zeros_like(singles[0][1])
    dep = np.zeros_like(singles[0][2])
    inst = np.full(dep.shape, -1, np.int32)
    for i, (r, n, d) in enumerate(singles):
        take = (d > 0) & ((inst < 0) | (d < dep))
        rgb[take], nrm[take], dep[take], inst[take] = r[take], n[take], d[take], i
    return rgb, nrm, dep, inst


def test_multi_object_scenes_at_msaa1_equal_the_nearest_composite_of_oracle_renders(engine_meshes):
    from oracle import raster as orr
    from tests.support import raster_scene as rsc

    h, w = 240, 320
    rng = np.random.RandomState(21)
    base = _poses(1, 12, z=(0.45, 0.45), xy=0.0)[0]
    poses = []
    for k in range(4):   # overlapping in the image, separated in depth (no interpenetration: no two surfaces at nearly equal depth)
        T = base.copy()
        T[:3, 3] += [0.06 * (k - 1.5), 0.02 * rng.randn(), 0.2 * k]
        poses.append(T)
    poses.append(poses[1].copy())   # an exact duplicate of object 1 (same mesh, same pose): every sample ties, object 1 must win
    mesh_ids = [0, 1, 2, 0, 1]
    lights = [[(0.3, -0.2, 0.1), (-0.5, 0.4, -0.3)], [(0.2, 0.2, 0.2)], [(0.0, -0.6, 0.2), (0.4, 0.0, 0.1), (0.1, 0.1, -0.5)], [(0.5, 0.5, 0.0)],
              [(0.2, 0.2, 0.2)]]
    rigs = [_oracle_rig(p, [(0.3, 0.25, 0.2)] * len(p)) for p in lights]
    T = np.stack(poses).astype(np.float32)
    flags = 3
    singles = [orr.render(engine_meshes[m], T[i:i + 1], K_HALF[None], h, w, flags, rigs[i]) for i, m in enumerate(mesh_ids)]
    singles = [(r[0], n[0], d[0]) for r, n, d in singles]
    rgb_c, nrm_c, dep_c, inst_c = _composite(singles)
    for reverse in (0, 1):   # (4) reversed tile lists: the same result
        rgb, nrm, dep, inst = rsc.render(engine_meshes, [0, 5], mesh_ids, T, K_HALF[None], [0.123], rigs, h, w, flags, reverse=reverse)
        assert np.array_equal(dep[0], dep_c) and np.array_equal(inst[0], inst_c)
        assert np.array_equal(rgb[0], rgb_c) and np.array_equal(nrm[0], nrm_c)
    seen = set(np.unique(inst_c).tolist()) - {-1}
    assert len(seen) >= 3 and 1 in seen and 4 not in seen, seen   # objects occlude each other; the duplicate never wins (ties -> first)
    assert (singles[4][2] > 0).sum() > 100


def test_disjoint_objects_at_msaa4_are_the_union_of_their_oracle_renders(engine_meshes):
    from oracle import raster as orr
    from tests.support import raster_scene as rsc

    h, w = 240, 320
    T = _poses(2, 13, z=(0.9, 0.9), xy=0.0).astype(np.float32)
    T[0, 0, 3], T[1, 0, 3] = -0.14, 0.14
    flags = 16 | 3
    rigs = [_oracle_rig([(0.3, 0.1, -0.2)], [(0.5, 0.4, 0.3)]), _oracle_rig([(-0.3, 0.2, 0.1), (0.0, 0.0, -0.4)], [(0.3, 0.3, 0.3)] * 2)]
    singles = [orr.render(engine_meshes[i], T[i:i + 1], K_HALF[None], h, w, flags, rigs[i]) for i in range(2)]
    tiles = []
    for r, _, _ in singles:
        ys, xs = np.nonzero((r[0] > 0).any(-1))
        tiles.append({(y // 8, x // 8) for y, x in zip(ys, xs)})
    assert tiles[0] and tiles[1] and not (tiles[0] & tiles[1]), "the objects' tile footprints must be disjoint"
    rgb, nrm, dep, inst = rsc.render(engine_meshes[:2], [0, 2], [0, 1], T, K_HALF[None], [0.2], rigs, h, w, flags)
    assert np.array_equal(rgb[0], singles[0][0][0] + singles[1][0][0])
    assert np.array_equal(nrm[0], singles[0][1][0] + singles[1][1][0])
    assert np.array_equal(dep[0], singles[0][2][0] + singles[1][2][0])
    assert np.array_equal(inst[0], np.where(singles[0][2][0] > 0, 0, np.where(singles[1][2][0] > 0, 1, -1)))


def test_empty_cameras_non_finite_pose_and_k_render_background(engine_meshes):
    from tests.support import raster_scene as rsc

    T = _poses(3, 14).astype(np.float32)
    T[1, 0, 0] = np.nan
    K = np.repeat(K_TINY[None], 3, 0)
    K[2, 0, 0] = np.inf
    rgb, nrm, dep, inst = rsc.render(engine_meshes, [0, 0, 2, 3, 4], [0, 1, 2, 0], np.concatenate([T, T[:1]]), np.concatenate([K, K[:1]]),
                                     [0.1] * 4, [_axis_rig()] * 4, 60, 80, 16 | 3)
    assert rgb[0].max() == 0 and dep[0].max() == 0 and (inst[0] == -1).all()   # no objects
    assert dep[1].max() > 0 and set(np.unique(inst[1]).tolist()) == {-1, 0}     # object 1 (non-finite pose) contributes nothing
    assert rgb[2].max() == 0 and (inst[2] == -1).all()                          # non-finite K
    assert dep[3].max() > 0
