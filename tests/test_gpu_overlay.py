"""GPU: the prediction overlays on the device (mp_overlay, mp_draw_boxes / megapose6d_amd.visualization) -- the kernels against their host
emulation (tests/overlay_emul.cpp, itself pinned to an independent restatement by tests/test_overlay_contract_cpu.py), every output byte,
exactly; the rejected arguments; and the public module end to end on a render of the scene renderer."""
import numpy as np
import pytest
import torch

from tests.support import overlay as ov

pytestmark = pytest.mark.gpu


def _shapes():
    """the shapes of the contract test and one more at the kernel's tile height + 1 and tile width + 1"""
    lim = ov.limits()
    return ov.SHAPES + ((lim["tile_h"] + 1, lim["tile_w"] + 1),)


def _dev(a):
    """a fresh device tensor of a (read-only) case array"""
    return None if a is None else torch.from_numpy(np.array(a)).cuda()


def _run(images, render, labels, k, outputs=ov.OUTPUTS, colors=ov.COLORS):
    from megapose6d_amd import engine as eng

    out = eng.overlay(_dev(images), render=_dev(render), labels=_dev(labels), colors=colors, dilate_iterations=k, outputs=outputs)
    assert set(out) == set(outputs)
    return {name: t.cpu().numpy() for name, t in out.items()}


def _assert_same(got, ref, what):
    assert set(got) == set(ref)
    for name in ref:
        assert got[name].dtype == np.uint8 and got[name].shape == ref[name].shape
        bad = np.argwhere(got[name] != ref[name])
        assert len(bad) == 0, f"{what}: {name} differs at {len(bad)} bytes, first {bad[0].tolist()}"


@pytest.mark.parametrize("mode", ("labels", "render"))
@pytest.mark.parametrize("k", (0, 1, 8))
def test_kernel_equals_the_emulation(k, mode):
    for h, w in _shapes():
        images, render, labels = ov.scene(2, h, w, 1)
        lab = labels if mode == "labels" else None
        _assert_same(_run(images, render, lab, k), ov.emul(images, render, lab, k=k), f"{h}x{w} k={k} {mode}")


def test_batch_with_a_background_image_and_every_set_of_outputs():
    images, render, labels = ov.batch3()
    full = ov.emul(images, render, labels, k=1)
    for bits in range(16):
        names = tuple(n for i, n in enumerate(ov.OUTPUTS) if bits >> i & 1)
        _assert_same(_run(images, render, labels, 1, outputs=names), {n: full[n] for n in names}, f"outputs {names}")
    # without a render: everything but the mesh
    _assert_same(_run(images, None, labels, 1, outputs=("contour", "canny", "mask")), {n: full[n] for n in ("contour", "canny", "mask")}, "no render")


def _shifted(a, fill=None):
    """a device tensor of a's shape that starts one byte into a 4-byte aligned buffer, holding a's bytes (or `fill`)"""
    buf = torch.full((a.size + 4,), 0xA5 if fill is None else fill, dtype=torch.uint8, device="cuda")
    t = buf[1:1 + a.size].view(a.shape)
    if fill is None:
        t.copy_(_dev(a))
    assert t.data_ptr() % 4 == 1 and t.is_contiguous()
    return t, buf


def test_tensors_that_are_not_dword_aligned_take_the_byte_path():
    """w % 4 == 0, so only the pointers decide: each of images, render and every output one byte off in turn, then all of them; through the
    C entry, because the binding allocates the outputs itself.  The bytes around a shifted output stay as they were."""
    from megapose6d_amd import _lib

    lib = _lib.load()
    images, render, labels = ov.batch3()
    want = ov.emul(images, render, labels, k=2)
    n, h, w = labels.shape
    colors, d_labels = _dev(ov.COLORS), _dev(labels)
    stream = torch.cuda.current_stream().cuda_stream
    names = ("contour", "canny", "mask", "mesh")
    for off in ({"images"}, {"render"}, {"contour"}, {"canny"}, {"mask"}, {"mesh"}, {"images", "render", *names}):
        ins = {k: (_shifted(a)[0] if k in off else _dev(a)) for k, a in (("images", images), ("render", render))}
        outs, bufs = {}, {}
        for name in names:
            if name in off:
                outs[name], bufs[name] = _shifted(want[name], fill=0x5A)
            else:
                outs[name] = torch.full(want[name].shape, 0x5A, dtype=torch.uint8, device="cuda")
        rc = lib.mp_overlay(ins["images"].data_ptr(), ins["render"].data_ptr(), d_labels.data_ptr(), colors.data_ptr(), len(ov.COLORS), n, h, w, 2,
                            *[outs[name].data_ptr() for name in names], stream)
        assert rc == 0
        _assert_same({name: t.cpu().numpy() for name, t in outs.items()}, want, f"one byte off: {sorted(off)}")
        for name, buf in bufs.items():
            rim = buf.cpu().numpy()
            assert rim[0] == 0x5A and (rim[1 + want[name].size:] == 0x5A).all(), f"{name}: a byte outside the output was written"


def test_an_output_that_is_not_asked_for_is_not_written():
    """through the C entry with all four buffers allocated and filled with 0xA5: for every subset of output pointers, the outputs asked for
    equal the emulation and the buffers whose pointer was not passed still hold 0xA5 everywhere"""
    from megapose6d_amd import _lib

    lib = _lib.load()
    images, render, labels = ov.batch3()
    want = ov.emul(images, render, labels, k=1)
    n, h, w = labels.shape
    d_images, d_render, d_labels, colors = _dev(images), _dev(render), _dev(labels), _dev(ov.COLORS)
    stream = torch.cuda.current_stream().cuda_stream
    names = ("contour", "canny", "mask", "mesh")
    for bits in range(16):
        asked = [name for i, name in enumerate(names) if bits >> i & 1]
        bufs = {name: torch.full(want[name].shape, 0xA5, dtype=torch.uint8, device="cuda") for name in names}
        rc = lib.mp_overlay(d_images.data_ptr(), d_render.data_ptr(), d_labels.data_ptr(), colors.data_ptr(), len(ov.COLORS), n, h, w, 1,
                            *[bufs[name].data_ptr() if name in asked else None for name in names], stream)
        assert rc == 0
        for name in names:
            got = bufs[name].cpu().numpy()
            if name in asked:
                assert np.array_equal(got, want[name]), f"asked {asked}: {name} differs"
            else:
                assert (got == 0xA5).all(), f"asked {asked}: {name} was written"


def test_rejected_arguments_return_non_zero():
    from megapose6d_amd import _lib
    from megapose6d_amd import engine as eng

    lib = _lib.load()
    images, render, labels = (_dev(a) for a in ov.scene(1, 13, 17, 1))
    colors = _dev(ov.COLORS)
    outs = [torch.full((1, 13, 17, c), 0xA5, dtype=torch.uint8, device="cuda") for c in (3, 1, 1, 3)]
    stream = torch.cuda.current_stream().cuda_stream

    def call(im=images, rn=render, lb=labels, co=colors, n_colors=5, n=1, h=13, w=17, k=1, out=(0, 1, 2, 3)):
        ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731
        return lib.mp_overlay(ptr(im), ptr(rn), ptr(lb), ptr(co), n_colors, n, h, w, k, *[outs[i].data_ptr() if i in out else None for i in range(4)], stream)

    assert call() == 0
    assert call(im=None) != 0 and call(co=None) != 0 and call(rn=None, lb=None, out=(0, 1, 2)) != 0
    assert call(rn=None) != 0, "the mesh blend without a render"
    assert call(rn=None, out=(0, 1, 2)) == 0
    assert call(k=-1) != 0 and call(k=9) != 0 and call(n_colors=0) != 0
    assert call(h=0) != 0 and call(w=0) != 0 and call(h=8193) != 0 and call(w=8193) != 0 and call(n=-1) != 0
    assert call(n=2 ** 20, h=32, w=32) != 0, "n * h * w * 3 = 2^30 * 3 is not below 2^31"
    assert call(n=0, im=None, k=99) == 0, "n = 0 is a no-op"
    boxes, ids = torch.zeros(2, 4, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda")

    def draw(im=images, bx=boxes, bi=ids, n_boxes=2, co=colors, n_colors=5, n=1, h=13, w=17, t=2, out=outs[0]):
        ptr = lambda t_: None if t_ is None else t_.data_ptr()   # noqa: E731
        return lib.mp_draw_boxes(ptr(im), ptr(bx), ptr(bi), n_boxes, ptr(co), n_colors, n, h, w, t, ptr(out), stream)

    assert draw() == 0 and draw(bx=None, bi=None, n_boxes=0) == 0 and draw(n=0, im=None, t=0) == 0
    assert draw(im=None) != 0 and draw(bx=None) != 0 and draw(bi=None) != 0 and draw(co=None) != 0 and draw(out=None) != 0
    assert draw(t=0) != 0 and draw(t=9) != 0 and draw(n_boxes=-1) != 0 and draw(n_colors=0) != 0 and draw(h=0) != 0 and draw(w=8193) != 0
    torch.cuda.synchronize()
    # the binding refuses the same before it calls
    for kwargs in (dict(dilate_iterations=9), dict(outputs=("mesh",), render=None), dict(outputs=("edges",)), dict(colors=np.zeros((0, 3), np.uint8))):
        args = dict(render=render, labels=labels, colors=ov.COLORS, outputs=("canny",))
        args.update(kwargs)
        with pytest.raises(eng.EngineError):
            eng.overlay(images, **args)
    with pytest.raises(eng.EngineError):
        eng.overlay(images, outputs=("canny",))
    with pytest.raises(eng.EngineError):
        eng.draw_boxes(images, boxes, ids, thickness=0)


@pytest.mark.parametrize("t", (1, 2, 8))
def test_draw_boxes_equals_the_emulation(t):
    from megapose6d_amd import engine as eng

    images, boxes, ids = ov.box_case()
    for im in (images, np.ascontiguousarray(images[:, :, :23])):   # w = 24: dword accesses; w = 23: bytes
        got = eng.draw_boxes(_dev(im), _dev(boxes), _dev(ids), colors=ov.COLORS, thickness=t)
        assert np.array_equal(got.cpu().numpy(), ov.emul_boxes(im, boxes, ids, t=t))
    # w = 24 with the images, then the output, one byte off a dword: bytes again (the output through the C entry: the binding allocates it)
    want = ov.emul_boxes(images, boxes, ids, t=t)
    got = eng.draw_boxes(_shifted(images)[0], _dev(boxes), _dev(ids), colors=ov.COLORS, thickness=t)
    assert np.array_equal(got.cpu().numpy(), want)
    from megapose6d_amd import _lib

    out, buf = _shifted(images, fill=0x5A)
    d_images, d_boxes, d_ids, colors = _dev(images), _dev(boxes), _dev(ids), _dev(ov.COLORS)
    rc = _lib.load().mp_draw_boxes(d_images.data_ptr(), d_boxes.data_ptr(), d_ids.data_ptr(), len(ids), colors.data_ptr(), len(ov.COLORS),
                                   *images.shape[:3], t, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0 and np.array_equal(out.cpu().numpy(), want)
    rim = buf.cpu().numpy()
    assert rim[0] == 0x5A and (rim[1 + images.size:] == 0x5A).all()
    none = eng.draw_boxes(_dev(images), torch.zeros(0, 4).cuda(), torch.zeros(0, dtype=torch.int32).cuda(), colors=ov.COLORS, thickness=t)
    assert np.array_equal(none.cpu().numpy(), images)


def test_draw_boxes_lists_the_kept_boxes_in_order_across_waves_and_chunks():
    """259 boxes on two images of 20 x 24 (one chunk of 256 and one of 3; tiles of 16 rows): the kept boxes of a tile are listed in
    ascending order from all four waves.  `some`: 65 scattered boxes belong to image 0 and lie in rows 1 .. 13 (65 kept in its upper tile,
    none in its lower one), the other 194 to image 1 and far outside it (none kept).  `every`: all 259 belong to image 0 and cross row 16
    (every box kept in both of its tiles).  Every byte against the emulation."""
    from megapose6d_amd import engine as eng

    images, _, _ = ov.box_case()
    n, rng = 259, np.random.RandomState(7)
    x1, y1 = rng.uniform(-2, 14, n), rng.uniform(1, 8, n)
    some = np.stack([x1, y1, x1 + rng.uniform(2, 12, n), y1 + rng.uniform(1, 5, n)], 1).astype(np.float32)
    ids = np.ones(n, np.int32)
    ids[rng.permutation(n)[:65]] = 0
    some[ids == 1] += np.float32(200.0)
    assert some[ids == 0, 3].max() < 14 and (ids == 0).sum() == 65
    every = np.stack([x1, y1, x1 + rng.uniform(2, 12, n), rng.uniform(16, 19, n)], 1).astype(np.float32)
    for boxes, box_ids in ((some, ids), (every, np.zeros(n, np.int32))):
        for t in (1, 2):
            got = eng.draw_boxes(_dev(images), _dev(boxes), _dev(box_ids), colors=ov.COLORS, thickness=t)
            want = ov.emul_boxes(images, boxes, box_ids, t=t)
            assert np.array_equal(got.cpu().numpy(), want) and not np.array_equal(want[0], images[0])
            assert np.array_equal(want[1], images[1])


@pytest.fixture(scope="module")
def rendered_scene(object_dataset):
    """two overlapping objects of the test meshes at 96 x 128 under the white ambient light of the reference's script"""
    from megapose6d_amd import Panda3dSceneRenderer
    from megapose6d_amd.types import Panda3dLightData

    scene = Panda3dSceneRenderer(object_dataset)
    labels = [o.label for o in object_dataset.list_objects][:2]
    c, s = np.cos(1.2), np.sin(1.2)
    T = np.repeat(np.eye(4, dtype=np.float32)[None], 2, 0)
    T[:, :3, :3] = np.asarray([[1, 0, 0], [0, c, -s], [0, s, c]], np.float32)
    T[0, :3, 3] = (0.0, 0.0, 0.5)
    T[1, :3, 3] = (0.025, 0.01, 0.62)
    K = np.asarray([[150.0, 0, 64.0], [0, 150.0, 48.0], [0, 0, 1]], np.float32)
    r = scene.render_scenes(labels, torch.from_numpy(T).cuda(), torch.from_numpy(np.repeat(K[None], 2, 0)).cuda(), [0, 0], (96, 128),
                            [Panda3dLightData(light_type="ambient", color=(1.0, 1.0, 1.0, 1))])
    rgb = np.random.RandomState(9).randint(0, 256, size=(96, 128, 3)).astype(np.uint8)
    yield scene, labels, T, K, r, rgb
    scene.close()


def test_overlay_scenes_equals_the_emulation_on_a_scene_render(rendered_scene):
    from megapose6d_amd import visualization as vis

    scene, labels, T, K, r, rgb = rendered_scene
    inst = r.instance_ids.cpu().numpy()
    assert set(np.unique(inst).tolist()) == {-1, 0, 1}
    a, b = inst[0][:, :-1], inst[0][:, 1:]
    assert ((a >= 0) & (b >= 0) & (a != b)).any(), "the two objects must overlap in the image"
    render = torch.round(r.rgbs * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous().cpu().numpy()
    got = vis.overlay_scenes(rgb, r, dilate_iterations=1)
    assert all(t.is_cuda and t.dtype == torch.uint8 for t in got.values())
    want = ov.emul(rgb[None], render, inst, colors=np.asarray(vis.DEFAULT_PALETTE, np.uint8), k=1)
    _assert_same({n: t.cpu().numpy() for n, t in got.items()}, want, "overlay_scenes")
    painted = got["contour"][0].cpu().numpy()[want["canny"][0] > 0]
    assert {tuple(c) for c in painted.tolist()} == {vis.DEFAULT_PALETTE[0], vis.DEFAULT_PALETTE[1]}, "each object has its own colour"


def test_output_visualization_is_the_reference_picture(rendered_scene, tmp_path):
    from megapose6d_amd import visualization as vis

    scene, labels, T, K, r, rgb = rendered_scene
    render = torch.round(r.rgbs * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous().cpu().numpy()[0]
    ref = vis.make_contour_overlay(rgb, render)
    assert ref["mask"].dtype == np.bool_ and ref["canny"].dtype == np.uint8 and set(np.unique(ref["canny"]).tolist()) == {0, 255}
    want = ov.emul(rgb[None], render[None], None, colors=np.asarray([[0, 255, 0]], np.uint8), k=1)
    assert np.array_equal(ref["img"], want["contour"][0]) and np.array_equal(ref["canny"], want["canny"][0])
    assert np.array_equal(ref["mask"], want["mask"][0] > 0) and np.array_equal(ref["mask"], (render > 0).any(-1))
    out = vis.make_output_visualization(rgb, labels, T, K, scene, per_instance=False)
    assert np.array_equal(out["contour_overlay"], ref["img"])
    assert np.array_equal(out["mesh_overlay"], vis.make_mesh_overlay(rgb, render)) and np.array_equal(out["mesh_overlay"], want["mesh"][0])
    assert np.array_equal(out["rgb"], rgb)
    assert np.array_equal(out["all_results"], np.concatenate([rgb, out["contour_overlay"], out["mesh_overlay"]], 1))
    red = vis.make_contour_overlay(rgb, render, color=(255, 0, 0), dilate_iterations=0)
    assert (red["img"][red["canny"] > 0] == (255, 0, 0)).all() and (red["canny"] > 0).sum() < (ref["canny"] > 0).sum()
    per = vis.make_output_visualization(rgb, labels, T, K, scene, per_instance=True)
    assert np.array_equal(per["contour_overlay"], vis.overlay_scenes(rgb, r)["contour"][0].cpu().numpy())
    written = vis.save_visualizations(tmp_path / "visualizations", out)
    assert sorted(p.name for p in written) == ["all_results.png", "contour_overlay.png", "mesh_overlay.png"]
    from PIL import Image

    assert np.array_equal(np.asarray(Image.open(tmp_path / "visualizations" / "contour_overlay.png")), out["contour_overlay"])


def test_draw_detections_on_a_collection():
    import pandas as pd

    from megapose6d_amd import visualization as vis
    from megapose6d_amd.tcoll import PandasTensorCollection

    images, boxes, ids = ov.box_case()
    det = PandasTensorCollection(infos=pd.DataFrame(dict(label=["o"] * len(ids), batch_im_id=ids, instance_id=np.arange(len(ids)))),
                                 bboxes=torch.from_numpy(np.array(boxes)))
    got = vis.draw_detections(images, det)
    assert isinstance(got, np.ndarray) and np.array_equal(got, ov.emul_boxes(images, boxes, ids, colors=np.asarray([[255, 0, 0]], np.uint8), t=2))
    got = vis.draw_detections(_dev(images), det, colors=ov.COLORS, thickness=1)
    assert got.is_cuda and np.array_equal(got.cpu().numpy(), ov.emul_boxes(images, boxes, ids, t=1))
