"""GPU: the multi-object scene renderer on the device (mp_raster_render_scene / Panda3dSceneRenderer) -- the kernel against its host
emulation (tests/raster_scene_emul.cpp, itself pinned to the oracle by tests/test_scene_renderer_cpu.py) bit for bit, the tie to the
pinned single-object path (Panda3dBatchRenderer), and the reference-API wrapper."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

K_FULL = np.array([[605.95, 0, 319.03], [0, 605.0, 249.68], [0, 0, 1]], np.float32)


def _poses(n, seed, z=(0.45, 0.8), xy=0.3):
    from tests.support import synthetic as syn

    rng = np.random.RandomState(seed)
    return np.stack([syn.random_pose(rng, z_range=z, xy_frac=xy) for _ in range(n)])


@pytest.fixture(scope="module")
def scene_meshes(engine_meshes, tmp_path_factory):
    from megapose6d_amd import mesh_io
    from tests.support import synthetic as syn

    tex = mesh_io.load_rigid_object(syn.make_textured_object(tmp_path_factory.mktemp("tex"), fmt="obj"))
    return [tex] + list(engine_meshes)


def _scene_rigs(n):
    """make_scene_lights()' rig in the engine form (dir = +-axes, offset 0), plus an offset light, per object"""
    from megapose6d_amd import engine as eng
    from megapose6d_amd.types import _POINT_DIRS

    dirs = list(_POINT_DIRS) + [(0.0, 0.0, 0.0)]
    offs = [(0.0, 0.0, 0.0)] * 6 + [(0.05, -0.1, 0.2)]
    cols = [(0.4, 0.4, 0.4)] * 6 + [(0.2, 0.1, 0.3)]
    return [eng.make_lights((0.1, 0.1, 0.1), dirs, cols, offs) for _ in range(n)]


@pytest.mark.parametrize("msaa", [1, 4])
def test_kernel_equals_host_emulation_on_overlapping_scenes(scene_meshes, msaa):
    from megapose6d_amd import engine as eng
    from tests.support import raster_scene as rsc

    h, w = 480, 640
    db = eng.MeshDB(scene_meshes)
    try:
        # camera 0: 7 overlapping objects (textured + vertex-coloured, one with a non-finite pose, one crossing the near plane);
        # camera 1: no object; camera 2: 3 objects, one exact duplicate (depth ties)
        T0 = _poses(7, 31, z=(0.4, 0.7), xy=0.12)
        T0[5, 0, 0] = np.nan
        T0[6] = _poses(1, 32, z=(0.08, 0.11), xy=0.05)[0]
        T0[6][0, 3] += 0.07   # (to the right: it covers a third of the frame, not all of it)
        T2 = _poses(2, 33, z=(0.5, 0.6), xy=0.05)
        T = np.concatenate([T0, T2, T2[:1]]).astype(np.float32)
        mesh_ids = [0, 1, 2, 3, 0, 1, 2, 0, 3, 0]
        obj_off = [0, 7, 7, 10]
        K = np.repeat(K_FULL[None], 3, 0)
        radius = np.array([0.21, 0.3, 0.17], np.float32)
        rigs = _scene_rigs(len(mesh_ids))
        dev = torch.device("cuda")
        for gl in (0, 4):
            flags = 3 | gl | (16 if msaa == 4 else 0)
            out = torch.full((3, h, w, 8), -7.0, device=dev)
            inst = torch.full((3, h, w), -7, dtype=torch.int32, device=dev)
            eng.raster_render_scene(db, obj_off, torch.tensor(mesh_ids, dtype=torch.int32, device=dev), torch.from_numpy(T).to(dev),
                                    torch.from_numpy(K).to(dev), torch.from_numpy(radius).to(dev), eng.lights_array(rigs, dev), h, w, flags, out,
                                    h * w * 8, w * 8, 8, 0, 3, 6, inst)
            torch.cuda.synchronize()
            o = out.cpu().numpy()
            rgb, nrm, dep, ins = rsc.render(scene_meshes, obj_off, mesh_ids, T, K, radius, rigs, h, w, flags)
            assert (o[..., 7] == -7.0).all()   # the unwritten channel stays untouched
            assert np.array_equal(o[..., 0:3], rgb), ("rgb", (o[..., 0:3] != rgb).mean())
            assert np.array_equal(o[..., 3:6], nrm), ("normals", (o[..., 3:6] != nrm).mean())
            assert np.array_equal(o[..., 6], dep)
            assert np.array_equal(inst.cpu().numpy(), ins)
        assert o[1, ..., :7].max() == 0 and (ins[1] == -1).all()
        seen = set(np.unique(ins[0]).tolist())
        assert seen == {-1, 0, 1, 2, 3, 4, 6}, seen   # every finite object wins somewhere; the non-finite pose never does
        assert dep[0][ins[0] == 6].min() < 0.1 + 1e-4   # the near-plane crossing object is clipped at z = 0.1
        assert 2 not in set(np.unique(ins[2]).tolist())            # the duplicate of object 0 never wins a tie
    finally:
        db.close()


@pytest.fixture(scope="module")
def renderers(object_dataset):
    from megapose6d_amd import Panda3dBatchRenderer, Panda3dSceneRenderer

    out = {m: (Panda3dSceneRenderer(object_dataset, msaa=m), Panda3dBatchRenderer(object_dataset, n_workers=1, msaa=m)) for m in (1, 4)}
    yield out
    for s, b in out.values():
        s.close()
        b.stop()


@pytest.mark.parametrize("msaa", [1, 4])
def test_one_object_scene_at_identity_equals_the_batch_renderer(renderers, object_dataset, msaa):
    from megapose6d_amd.scene_renderer import scene_tco
    from megapose6d_amd.types import Panda3dCameraData, Panda3dObjectData, make_scene_lights

    scene, batch = renderers[msaa]
    labels = [o.label for o in object_dataset.list_objects]
    T = _poses(3, 41, z=(0.4, 0.6), xy=0.1)
    lights = make_scene_lights()
    for i, lab in enumerate(labels):
        TWC = np.linalg.inv(T[i])
        r = scene.render_scene([Panda3dObjectData(lab)], [Panda3dCameraData(K=K_FULL, resolution=(480, 640), TWC=TWC)], lights,
                               render_depth=True, render_normals=True)[0]
        TCO = scene_tco(TWC, np.eye(4)).astype(np.float32)   # the pose the scene path composes (float64, rounded once)
        b = batch.render([lab], torch.from_numpy(TCO[None]).cuda(), torch.from_numpy(K_FULL[None]).cuda(), [lights], (480, 640),
                         render_depth=True, render_normals=True)
        rgb = torch.round(b.rgbs[0] * 255).to(torch.uint8).permute(1, 2, 0).cpu().numpy()
        nrm = torch.round(b.normals[0] * 255).to(torch.uint8).permute(1, 2, 0).cpu().numpy()
        dep = b.depths[0].permute(1, 2, 0).cpu().numpy()
        assert (dep > 0).mean() > 0.01
        assert np.array_equal(r.rgb, rgb) and np.array_equal(r.normals, nrm) and np.array_equal(r.depth, dep)


def test_render_scene_api(renderers, object_dataset):
    from megapose6d_amd.types import CameraRenderingData, Panda3dCameraData, Panda3dObjectData, make_scene_lights

    scene, _ = renderers[4]
    labels = [o.label for o in object_dataset.list_objects]
    T = _poses(4, 51, z=(0.45, 0.6), xy=0.15)
    objs = [Panda3dObjectData(labels[i % 3], TWO=T[i]) for i in range(4)]
    K_small = np.array([[300.0, 0, 160.5], [0, 300.0, 119.5], [0, 0, 1]])
    cams = [Panda3dCameraData(K=K_FULL, resolution=(480, 640)), Panda3dCameraData(K=K_small, resolution=(240, 320)),
            Panda3dCameraData(K=K_FULL, resolution=(480, 640), TWC=np.linalg.inv(T[0]) @ np.linalg.inv(T[0]))]
    lights = make_scene_lights()
    res = scene.render_scene(objs, cams, lights, render_depth=True, render_binary_mask=True, render_normals=True)
    assert len(res) == 3 and all(isinstance(r, CameraRenderingData) for r in res)
    for r, c in zip(res, cams):
        h, w = c.resolution
        assert r.rgb.dtype == np.uint8 and r.rgb.shape == (h, w, 3)
        assert r.normals.dtype == np.uint8 and r.normals.shape == (h, w, 3)
        assert r.depth.dtype == np.float32 and r.depth.shape == (h, w, 1)
        assert r.binary_mask.dtype == np.bool_ and np.array_equal(r.binary_mask, r.depth[..., 0] > 0)
    assert res[0].binary_mask.mean() > 0.01 and res[1].binary_mask.mean() > 0.01
    assert set(scene.debug_data.timings) >= {"setup_time", "render_time"}
    # camera at the world origin: render_scene == the tensor path (rgb = round(resolved * 255))
    t = scene.render_scenes([o.label for o in objs], torch.from_numpy(T).cuda(), torch.from_numpy(np.repeat(K_FULL[None], 4, 0)).cuda(), [0] * 4,
                            (480, 640), lights, render_depth=True, render_normals=True)
    assert np.array_equal(res[0].rgb, torch.round(t.rgbs[0] * 255).to(torch.uint8).permute(1, 2, 0).cpu().numpy())
    assert np.array_equal(res[0].depth[..., 0], t.depths[0, 0].cpu().numpy())
    ins = t.instance_ids[0].cpu().numpy()
    assert np.array_equal(ins >= 0, res[0].depth[..., 0] > 0) and len(set(np.unique(ins).tolist()) - {-1}) >= 2
    # without depth: no mask
    r = scene.render_scene(objs[:1], cams[:1], lights)[0]
    assert r.depth is None and r.normals is None and r.binary_mask is None and r.rgb.shape == (480, 640, 3)


def test_render_scenes_groups_rows_like_separate_calls(renderers, object_dataset):
    from megapose6d_amd.types import make_scene_lights

    scene, _ = renderers[4]
    labels_all = [o.label for o in object_dataset.list_objects]
    T = torch.from_numpy(_poses(7, 61, z=(0.45, 0.7), xy=0.2)).cuda()
    K = torch.from_numpy(np.repeat(K_FULL[None], 7, 0)).cuda()
    labels = [labels_all[i % 3] for i in range(7)]
    sid = torch.tensor([2, 0, 2, 1, 0, 2, 0])
    lights = make_scene_lights()
    allr = scene.render_scenes(labels, T, K, sid, (240, 320), lights, render_depth=True, render_normals=True)
    assert allr.rgbs.shape == (3, 3, 240, 320) and allr.depths.shape == (3, 1, 240, 320) and allr.instance_ids.dtype == torch.int32
    for s in range(3):
        rows = [i for i in range(7) if int(sid[i]) == s]
        one = scene.render_scenes([labels[i] for i in rows], T[rows], K[rows], [0] * len(rows), (240, 320), lights, render_depth=True,
                                  render_normals=True)
        for a, b in ((allr.rgbs[s], one.rgbs[0]), (allr.normals[s], one.normals[0]), (allr.depths[s], one.depths[0]),
                     (allr.instance_ids[s], one.instance_ids[0])):
            assert torch.equal(a, b)
