"""GPU: the training-free detector on the device (mp_tm_quantize, mp_tm_response, mp_tm_match / megapose6d_amd.template_detector) -- the
kernels against their host emulation (tests/template_match_emul.cpp, itself pinned to an independent restatement by
tests/test_template_match_contract_cpu.py), every byte, exactly; unaligned inputs; guarded outputs; the rejected arguments; and the
public path from `make_template_detector` to `run_inference_pipeline`."""
import numpy as np
import pytest
import torch

from tests.support import template_match as tmm

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def _same(got, ref, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.dtype == ref.dtype and got.shape == ref.shape, (what, got.dtype, ref.dtype, got.shape, ref.shape)
    bad = np.argwhere(got != ref)
    assert len(bad) == 0, f"{what}: differs at {len(bad)} entries, first {bad[0].tolist()}"


def _run_chain(images, T, templates, features, n_objects, blur=True):
    from megapose6d_amd import engine as eng

    ori, mag2 = eng.tm_quantize(_dev(images), blur=blur, weak_threshold=tmm.WEAK)
    resp = eng.tm_response(ori, T)
    h, w = images.shape[1:3]
    out = eng.tm_match(resp, h, w, _dev(np.asarray(templates, np.int32).reshape(-1, 5)), _dev(np.asarray(features, np.uint8).reshape(-1, 4)), n_objects,
                       templates, features)
    return (ori, mag2, resp) + out


def _emul_chain(images, T, templates, features, n_objects, blur=True):
    ori, mag2 = tmm.emul_quantize(images, blur)
    resp = tmm.emul_response(ori, T)
    h, w = images.shape[1:3]
    return (ori, mag2, resp) + tmm.emul_match(resp, h, w, T, templates, features, n_objects)


NAMES = ("ori", "mag2", "resp", "best_score", "best_f", "best_template")


# ---- 1. kernels = emulation --------------------------------------------------------------------------------------------------------------
def _shapes():
    """the shapes of the contract test; one image at the quantise kernel's tile + 1 in each dimension; one whose location map at T = 1 is
    wider than a workgroup's location tile (and than the response kernel's tile) by one and one row higher"""
    lim = tmm.limits()
    return tmm.SHAPES + ((lim["quant_tile_h"] + 1, lim["quant_tile_w"] + 1), (lim["loc_h"] + 1, lim["loc_w"] + 1), (lim["resp_tile_h"] + 1, tmm.resp_tile(1)[0] + 1))


@pytest.mark.parametrize("blur", (True, False))
def test_kernels_equal_the_emulation(blur):
    for h, w in _shapes():
        images = tmm.image_case(2, h, w, 1)
        templates, features = tmm.table_case(h, w, 65, 1)
        for T in tmm.SPREADS:
            got = _run_chain(images, T, templates, features, tmm.N_OBJECTS, blur)
            for name, a, b in zip(NAMES, got, _emul_chain(images, T, templates, features, tmm.N_OBJECTS, blur)):
                _same(a, b, f"{name} {h}x{w} T={T} blur={blur}")


def test_limits_equal_the_emulation():
    for name, images, T, templates, features, n_objects in tmm.limit_cases():
        got = _run_chain(images, T, templates, features, n_objects)
        for what, a, b in zip(NAMES, got, _emul_chain(images, T, templates, features, n_objects)):
            _same(a, b, f"{what}: {name}")
    from megapose6d_amd import engine as eng

    none = torch.zeros((0, 13, 17, 3), dtype=torch.uint8, device="cuda")
    ori, mag2 = eng.tm_quantize(none)
    resp = eng.tm_response(ori, 5)
    templates, features = tmm.table_case(13, 17, 2, 1)
    out = eng.tm_match(resp, 13, 17, _dev(templates), _dev(features), 2, templates, features)
    assert ori.shape == (0, 13, 17) and resp.shape == (0, 8, 5, 5, 3, 4) and all(t.shape == (0, 2, 3, 4) for t in out)


# ---- 2. / 3. unaligned inputs, guarded outputs -------------------------------------------------------------------------------------------
GUARD = 256


def _guarded(ref: np.ndarray, fill: int, shift: int = 0):
    """a device tensor of ref's shape and dtype inside a buffer filled with `fill`, GUARD (+ shift) bytes from its start -> tensor, buffer"""
    nbytes = ref.size * ref.itemsize
    buf = torch.full((2 * GUARD + nbytes + 4,), fill, dtype=torch.uint8, device="cuda")
    t = buf[GUARD + shift:GUARD + shift + nbytes].view(torch.from_numpy(ref[:0].copy()).dtype).view(ref.shape)
    assert t.data_ptr() % 4 == (buf.data_ptr() + shift) % 4 and t.is_contiguous()
    return t, buf


def _shifted_copy(a: np.ndarray):
    """a device tensor holding a's bytes that starts one byte off a 4-byte boundary"""
    t, buf = _guarded(a, 0xA5, shift=1)
    t.copy_(_dev(a))
    assert t.data_ptr() % 4 == 1
    return t, buf


def _rim_intact(buf, fill, nbytes, shift=0):
    rim = buf.cpu().numpy()
    return (rim[:GUARD + shift] == fill).all() and (rim[GUARD + shift + nbytes:] == fill).all()


@pytest.mark.parametrize("shift", (0, 1))
def test_outputs_are_written_whole_and_nothing_around_them(shift):
    """through the C entries: every output inside a guarded buffer, pre-filled with 0xA5 and then with 0x5A (so that a byte left unwritten
    differs from the emulation in one of the two runs); shift 1: every byte tensor, inputs and outputs, starts one byte off a 4-byte
    boundary, and the templates' first features are odd offsets into the feature table (table_case leaves gaps of 0 .. 2 features)"""
    from megapose6d_amd import _lib

    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    images = tmm.image_case(3, 48, 64, 3)
    n, h, w = images.shape[:3]
    T = 5
    templates, features = tmm.table_case(h, w, 65, 2)
    assert (templates[:, 1] % 2 == 1).any() and (templates[:, 1] % 4 == 3).any(), "uneven feature-table offsets"
    want = dict(zip(NAMES, _emul_chain(images, T, templates, features, tmm.N_OBJECTS)))
    d_templates = _dev(templates)
    for fill in (0xA5, 0x5A):
        d_images, d_features = (_shifted_copy(images)[0], _shifted_copy(features)[0]) if shift else (_dev(images), _dev(features))
        out = {name: _guarded(want[name], fill, shift if want[name].dtype == np.uint8 else 0) for name in NAMES}
        assert lib.mp_tm_quantize(d_images.data_ptr(), n, h, w, 1, tmm.WEAK, out["ori"][0].data_ptr(), out["mag2"][0].data_ptr(), stream) == 0
        assert lib.mp_tm_response(out["ori"][0].data_ptr(), n, h, w, T, out["resp"][0].data_ptr(), stream) == 0
        assert lib.mp_tm_match(out["resp"][0].data_ptr(), n, h, w, T, d_templates.data_ptr(), templates.ctypes.data, d_features.data_ptr(),
                               features.ctypes.data, len(templates), len(features), tmm.N_OBJECTS, out["best_score"][0].data_ptr(),
                               out["best_f"][0].data_ptr(), out["best_template"][0].data_ptr(), stream) == 0
        for name in NAMES:
            t, buf = out[name]
            _same(t, want[name], f"{name} fill={fill:#x} shift={shift}")
            s = shift if want[name].dtype == np.uint8 else 0
            assert _rim_intact(buf, fill, want[name].size * want[name].itemsize, s), f"{name}: a byte outside the output was written"
    # mag2 is optional: NULL leaves ori unchanged
    ori, buf = _guarded(want["ori"], 0xA5)
    assert lib.mp_tm_quantize(_dev(images).data_ptr(), n, h, w, 1, tmm.WEAK, ori.data_ptr(), None, stream) == 0
    _same(ori, want["ori"], "ori without mag2")


# ---- 4. rejected arguments ---------------------------------------------------------------------------------------------------------------
def test_rejected_arguments_give_a_status_and_no_launch():
    from megapose6d_amd import _lib
    from megapose6d_amd import engine as eng

    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    images = _dev(tmm.image_case(1, 13, 17, 4))
    ori = torch.full((1, 13, 17), 0xA5, dtype=torch.uint8, device="cuda")
    mag2 = torch.full((1, 13, 17), 7, dtype=torch.int32, device="cuda")
    resp = torch.full((1, 8, 2, 2, 7, 9), 0xA5, dtype=torch.uint8, device="cuda")
    outs = [torch.full((1, 2, 7, 9), 0xA5, dtype=torch.uint8, device="cuda"), torch.full((1, 2, 7, 9), 0xA5, dtype=torch.uint8, device="cuda"),
            torch.full((1, 2, 7, 9), 7, dtype=torch.int32, device="cuda")]
    ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731

    def quantize(im=images, n=1, h=13, w=17, weak=30, o=ori):
        return lib.mp_tm_quantize(ptr(im), n, h, w, 1, weak, ptr(o), ptr(mag2), stream)

    assert quantize(im=None) != 0 and quantize(o=None) != 0 and quantize(h=0) != 0 and quantize(w=8193) != 0 and quantize(n=-1) != 0
    assert quantize(weak=-1) != 0 and quantize(weak=1444) != 0 and quantize(n=2 ** 20, h=32, w=32) != 0
    assert quantize(n=0, im=None) == 0

    def response(o=ori, n=1, h=13, w=17, T=2, r=resp):
        return lib.mp_tm_response(ptr(o), n, h, w, T, ptr(r), stream)

    assert response(o=None) != 0 and response(r=None) != 0 and response(T=0) != 0 and response(T=9) != 0 and response(h=0) != 0
    assert response(n=2 ** 14, h=128, w=128, T=1) != 0, "n * h * w * 3 is below 2^31, the maps of 2^31 bytes are not"
    assert response(n=0, o=None) == 0
    feats = np.zeros((70, 4), np.uint8)
    feats[:, :2] = 3
    d_feats = _dev(feats)

    def match(table, r=resp, n=1, h=13, w=17, T=2, features=feats, d_features=d_feats, n_objects=2, out=(0, 1, 2), host=True, n_templates=None):
        table = np.asarray(table, np.int32).reshape(-1, 5)
        d_table = _dev(table) if len(table) else None
        return lib.mp_tm_match(ptr(r), n, h, w, T, ptr(d_table), table.ctypes.data if host else None, ptr(d_features), features.ctypes.data if host else None,
                               len(table) if n_templates is None else n_templates, len(features), n_objects, *[ptr(outs[i]) if i in out else None for i in range(3)],
                               stream)

    ok = [[0, 0, 1, 4, 4]]
    assert match(ok, n=0, r=None) == 0
    assert match(ok, r=None) != 0 and match(ok, out=(0, 1)) != 0 and match(ok, host=False) != 0 and match(ok, d_features=None) != 0
    assert match(ok, T=0) != 0 and match(ok, T=9) != 0 and match(ok, n_objects=0) != 0 and match(ok, n_objects=65536) != 0 and match(ok, n_templates=-1) != 0
    assert match([[0, 0, 0, 4, 4]]) != 0 and match([[0, 0, 64, 4, 4]]) != 0, "f = 0 and f = 64"
    assert match([[0, 0, 1, 3, 4]]) != 0 and match([[0, 0, 1, 4, 3]]) != 0, "a feature outside its template's box"
    assert match([[0, 69, 2, 4, 4]]) != 0 and match([[0, -1, 1, 4, 4]]) != 0 and match([[2, 0, 1, 4, 4]]) != 0 and match([[0, 0, 1, 257, 4]]) != 0
    torch.cuda.synchronize()
    # nothing was launched: every buffer still holds its fill
    assert (ori == 0xA5).all() and (mag2 == 7).all() and (resp == 0xA5).all() and (outs[0] == 0xA5).all() and (outs[1] == 0xA5).all() and (outs[2] == 7).all()
    # the bindings refuse the same before they call, or pass the entry's status on
    for call in (lambda: eng.tm_quantize(images.float()), lambda: eng.tm_quantize(images[..., :2]), lambda: eng.tm_quantize(images, weak_threshold=1444),
                 lambda: eng.tm_quantize(images.cpu()), lambda: eng.tm_response(ori, 0), lambda: eng.tm_response(ori, 9), lambda: eng.tm_response(ori[0], 2),
                 lambda: eng.tm_match(resp, 13, 19, _dev(np.asarray(ok, np.int32)), d_feats, 2, np.asarray(ok, np.int32), feats),
                 lambda: eng.tm_match(resp, 13, 17, _dev(np.asarray(ok, np.int32)), d_feats, 0, np.asarray(ok, np.int32), feats),
                 lambda: eng.tm_match(resp, 13, 17, _dev(np.asarray(ok, np.int32)), d_feats, 2, np.asarray(ok, np.int32), feats[:5]),
                 lambda: eng.tm_match(resp, 13, 17, _dev(np.asarray([[0, 0, 1, 3, 4]], np.int32)), d_feats, 2, np.asarray([[0, 0, 1, 3, 4]], np.int32), feats)):
        with pytest.raises(eng.EngineError):
            call()


# ---- 5. the public path ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def detector_scene(tmp_path_factory):
    from megapose6d_amd import Panda3dBatchRenderer, make_template_detector
    from megapose6d_amd.pose_estimator import load_SO3_grid
    from megapose6d_amd.types import Panda3dLightData
    from tests.support import synthetic as syn

    ds = syn.make_object_dataset(tmp_path_factory.mktemp("tm_meshes"), n_objects=2, seed=0)
    renderer = Panda3dBatchRenderer(ds, n_workers=1, preload_cache=True)
    detector = make_template_detector(ds, tmm.DET_K, tmm.DET_HW, viewpoints=tmm.DET_GRID, distances=tmm.DET_DISTANCES, renderer=renderer)
    labels = [o.label for o in ds.list_objects]
    R = load_SO3_grid(tmm.DET_GRID).numpy()
    K = torch.from_numpy(tmm.DET_K).cuda()
    queries = []
    for seed, plant in tmm.DET_SCENES:
        poses = tmm.det_query_poses(R, seed, plant)
        objs = sorted(poses)
        out = renderer.render([labels[o] for o in objs], torch.from_numpy(np.stack([poses[o] for o in objs])).cuda(), K[None].repeat(len(objs), 1, 1),
                              [[Panda3dLightData("ambient", (1.0, 1.0, 1.0, 1.0))]] * len(objs), tmm.DET_HW, render_depth=True)
        rgb = torch.round(out.rgbs.clamp(0, 1) * 255).to(torch.uint8).permute(0, 2, 3, 1).cpu().numpy()
        masks = (out.depths[:, 0] > 0).cpu().numpy()
        image, boxes = tmm.det_compose(seed, plant, {o: rgb[i] for i, o in enumerate(objs)}, {o: masks[i] for i, o in enumerate(objs)})
        queries.append((seed, image, boxes))
    yield ds, labels, renderer, detector, queries
    renderer.stop()


def _observation(images_u8):
    from megapose6d_amd.types import ObservationTensor

    t = torch.from_numpy(np.stack(images_u8)).cuda().permute(0, 3, 1, 2).float() / 255
    return ObservationTensor(t.contiguous(), torch.from_numpy(tmm.DET_K)[None].repeat(len(images_u8), 1, 1).cuda())


def test_make_template_detector_finds_the_planted_objects(detector_scene):
    """the CONDITIONS of the CPU end-to-end test, on the engine's renderer and kernels, at the default threshold"""
    from megapose6d_amd import Detector
    from megapose6d_amd.template_detector import DEFAULT_THRESHOLD

    ds, labels, renderer, detector, queries = detector_scene
    model = detector.model
    ts = model.templates
    assert isinstance(detector, Detector) and model.threshold == DEFAULT_THRESHOLD
    assert len(ts) + ts.n_dropped == 2 * tmm.DET_GRID * len(tmm.DET_DISTANCES) and len(ts) >= 250 and ts.d_templates.is_cuda
    obs = _observation([q[1] for q in queries] + [np.array(tmm.det_background(q[0])) for q in queries])
    det = detector.get_detections(obs, output_masks=True)
    n = len(det)
    assert set(det.infos.columns) >= {"label", "score", "batch_im_id", "instance_id"} and det.bboxes.shape == (n, 4) and det.bboxes.is_cuda
    assert det.masks.shape == (n, *tmm.DET_HW) and det.masks.dtype == torch.bool
    boxes = det.bboxes.cpu().numpy()
    for i, (seed, image, planted) in enumerate(queries):
        for o, box in planted.items():
            rows = det.infos[(det.infos.batch_im_id == i) & (det.infos.label == labels[o])]
            hits = [(tmm.box_iou(box, boxes[r].tolist()), float(rows.score[r])) for r in rows.index]
            print(f"scene {seed} object {o}: box {box}, detections of its label (iou, similarity) {[(round(a, 3), round(s, 4)) for a, s in hits]}")
            assert any(a >= 0.5 for a, _ in hits), f"scene {seed}: object {o} has no detection with IoU >= 0.5 ({hits})"
        r = int(rows.index[int(np.argmax([a for a, _ in hits]))])
        m = det.masks[r].cpu().numpy()
        ys, xs = np.nonzero(m)
        assert m.any() and abs(xs.min() - boxes[r][0]) <= 1 and abs(ys.max() - boxes[r][3]) <= 1, "the mask is the silhouette at the box"
    background = det.infos[det.infos.batch_im_id >= len(queries)]
    sim = [float(s) for s in background.score]
    print(f"background detections: {sim}")
    assert len(background) == 0, "a background-only image yields no detection at the default threshold"
    # the highest background similarity, for the record
    raw = model.match(torch.from_numpy(np.stack([np.array(tmm.det_background(q[0])) for q in queries])).cuda())
    top = (raw[0].double() / (4 * raw[1].clamp(min=1)).double()).max().item()
    print(f"highest background similarity {top:.4f}")
    assert top < DEFAULT_THRESHOLD


def test_the_model_is_deterministic_and_feeds_the_pose_pipeline(detector_scene):
    from tests.support import scene

    ds, labels, renderer, detector, queries = detector_scene
    obs = _observation([queries[0][1]])
    images = [im for im in obs.images[:, :3]]
    a, b = detector.model(images), detector.model(images)
    assert len(a) == len(b) == 1 and len(a[0]["boxes"]) >= 2
    for key in ("boxes", "labels", "scores", "masks"):
        assert torch.equal(a[0][key], b[0][key]), key
    assert a[0]["masks"].shape == (len(a[0]["boxes"]), 1, *tmm.DET_HW) and a[0]["labels"].dtype == torch.int64
    u8 = (obs.images[:, :3] * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    raw_a, raw_b = detector.model.match(u8), detector.model.match(u8)
    assert all(torch.equal(x, y) for x, y in zip(raw_a, raw_b)), "identical bytes"
    est = scene.build_estimator(ds, SO3_grid_size=72)
    est.detector_model = detector
    det = detector.get_detections(obs, one_instance_per_class=True)
    final, extra = est.run_inference_pipeline(obs, detections=det.cuda(), n_refiner_iterations=1, n_pose_hypotheses=1)
    assert final.poses.shape == (len(det), 4, 4) and torch.isfinite(final.poses).all() and sorted(final.infos.label) == sorted(det.infos.label)
    again, _ = est.run_inference_pipeline(obs, run_detector=True, n_refiner_iterations=1, n_pose_hypotheses=1)
    assert len(again) >= len(final)
