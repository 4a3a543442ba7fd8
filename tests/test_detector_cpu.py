"""CPU: the detector row without a GPU -- the oracle's building blocks against known answers, the engine's
host-side checkpoint layout against the oracle's, the parameter tree of DetectorMaskRCNN, and the oracle pinned to its committed
golden outputs (tests/golden/detector_*.npz, written by oracle/make_detector_fixture.py)."""
from pathlib import Path

import numpy as np
import pytest
import torch

GOLD = Path(__file__).resolve().parent / "golden"


def test_engine_checkpoint_layout_equals_the_oracles_and_hosts_a_reference_state_dict():
    from megapose6d_amd import engine as eng
    from megapose6d_amd.mask_rcnn import DetectorMaskRCNN
    from oracle import mask_rcnn as om

    for n_classes in (2, 22):
        assert eng.DetectorNet.state_spec(n_classes) == [(n, tuple(s)) for n, s in om.state_spec(n_classes)]
    m = DetectorMaskRCNN(input_resize=(480, 640), n_classes=22)
    sd = {n: torch.zeros(s) for n, s in om.state_spec(22)}
    sd["backbone.body.bn1.num_batches_tracked"] = torch.tensor(0)   # BatchNorm2d-style checkpoints carry these counters
    assert not m.load_state_dict(sd, strict=True).missing_keys
    assert sorted(m.state_dict().keys()) == sorted(n for n, _ in om.state_spec(22))
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == dict(om.state_spec(22))
    # torchvision's layout: conv / linear tensors are parameters, FrozenBatchNorm2d terms are buffers
    params = {n for n, _ in m.named_parameters()}
    assert "backbone.body.conv1.weight" in params and "roi_heads.box_head.fc6.bias" in params
    assert "backbone.body.layer1.0.bn3.running_var" not in params and "backbone.body.layer2.0.downsample.1.weight" not in params
    assert m.min_size == 480 and m.max_size == 640
    with pytest.raises(NotImplementedError):
        m.train()(images=[torch.zeros(3, 8, 8)])
    with pytest.raises(AssertionError):
        DetectorMaskRCNN(backbone_str="resnet101-fpn")


def test_oracle_building_blocks_known_answers():
    from oracle import mask_rcnn as om

    # anchor_utils.py generate_anchors: the published base anchors of scale 32, ratios (0.5, 1, 2)
    assert om.base_anchors(32).tolist() == [[-23.0, -11.0, 23.0, 11.0], [-16.0, -16.0, 16.0, 16.0], [-11.0, -23.0, 11.0, 23.0]]
    a = om.grid_anchors([(2, 3)], (64, 96))[0]
    assert a.shape == (18, 4) and a[0].tolist() == [-23.0, -11.0, 23.0, 11.0] and a[3].tolist() == [9.0, -11.0, 55.0, 11.0]   # stride 32 in x
    assert a[9].tolist() == [-23.0, 21.0, 23.0, 43.0]                                                                     # second row: +32 in y
    # BoxCoder: zero deltas give the box back, unit dw doubles-by-e the width about the centre, dw is clamped at log(1000/16)
    b = torch.tensor([[10.0, 20.0, 30.0, 60.0]])
    assert torch.allclose(om.decode_boxes(torch.zeros(1, 4), b, (1, 1, 1, 1)), b)
    d = om.decode_boxes(torch.tensor([[0.0, 0.0, 1.0, 0.0]]), b, (1, 1, 1, 1))[0]
    assert abs((d[2] - d[0]).item() - 20 * np.e) < 1e-4 and abs(((d[0] + d[2]) / 2).item() - 20) < 1e-5
    big = om.decode_boxes(torch.tensor([[0.0, 0.0, 50.0, 0.0]]), b, (1, 1, 1, 1))[0]
    assert abs((big[2] - big[0]).item() - 20 * 1000 / 16) < 1e-2
    assert torch.allclose(om.decode_boxes(torch.tensor([[10.0, 0.0, 0.0, 0.0]]), b, (10, 10, 5, 5))[0, 0], torch.tensor(30.0))   # dx / 10 * width
    # NMS: greedy, IoU > thr suppresses, result ordered by decreasing score; brute-force check on random boxes
    g = torch.Generator().manual_seed(0)
    xy = torch.rand(60, 2, generator=g) * 50
    boxes = torch.cat([xy, xy + torch.rand(60, 2, generator=g) * 30 + 1], 1)
    scores = torch.rand(60, generator=g)
    keep = om.nms(boxes, scores, 0.5).tolist()
    order = scores.argsort(descending=True).tolist()
    ref = []
    for i in order:
        def iou(p, q):
            iw = max(0.0, min(p[2], q[2]) - max(p[0], q[0])); ih = max(0.0, min(p[3], q[3]) - max(p[1], q[1]))
            inter = iw * ih
            return inter / ((p[2] - p[0]) * (p[3] - p[1]) + (q[2] - q[0]) * (q[3] - q[1]) - inter)
        if all(iou(boxes[i].tolist(), boxes[j].tolist()) <= 0.5 for j in ref):
            ref.append(i)
    assert keep == ref
    lab = torch.randint(0, 3, (60,), generator=g)
    kb = om.batched_nms(boxes, scores, lab, 0.5)
    assert sorted(kb.tolist()) == sorted(sum([[int(torch.where(lab == c)[0][k]) for k in om.nms(boxes[lab == c], scores[lab == c], 0.5)] for c in range(3)], []))
    assert (scores[kb][:-1] >= scores[kb][1:]).all()
    # paste_masks_in_image: a constant mask fills its (1-pixel-padded, truncated) box and nothing else
    m = om.paste_masks(torch.ones(1, 1, 28, 28), torch.tensor([[4.0, 6.0, 12.0, 16.0]]), (24, 32))
    assert m.shape == (1, 1, 24, 32) and m[0, 0, 11, 8] == 1.0 and m[0, 0, 0, 0] == 0 and m[0, 0, 23, 31] == 0
    ys, xs = torch.nonzero(m[0, 0] > 0, as_tuple=True)
    assert xs.min() >= 3 and xs.max() <= 13 and ys.min() >= 5 and ys.max() <= 17
    # transform: the resize ratio is a float32 quotient (192 / 150 -> 191 rows), batches are padded to multiples of 32
    batch, sizes, orig = om.transform_images([torch.rand(3, 150, 200)], 192, 256)
    assert sizes == [(191, 255)] and orig == [(150, 200)] and batch.shape == (1, 3, 192, 256) and batch[0, :, 191].abs().max() == 0
    batch, sizes, _ = om.transform_images([torch.rand(3, 96, 128)], 96, 128)
    assert sizes == [(96, 128)] and batch.shape == (1, 3, 96, 128)


def test_oracle_is_pinned_to_its_golden_outputs():
    """the committed goldens are what the GPU test compares the engine with; the oracle must still produce them"""
    from oracle import mask_rcnn as om

    g = np.load(GOLD / "detector_native.npz")
    n, H, W, mn, mx, C = (int(v) for v in g["config"])
    torch.set_num_threads(min(16, torch.get_num_threads() if torch.get_num_threads() > 1 else 16))
    out, dbg = om.mask_rcnn_forward(om.synthetic_state_dict(C), list(om.synthetic_images(n, H, W)), mn, mx, return_intermediates=True)
    k = int(g["counts"][0])
    assert len(out[0]["boxes"]) == k
    assert np.abs(out[0]["boxes"].numpy() - g["boxes"][0, :k]).max() < 1e-3 and np.abs(out[0]["scores"].numpy() - g["scores"][0, :k]).max() < 1e-5
    assert (out[0]["labels"].numpy() == g["labels"][0, :k]).all()
    for l in range(2, 7):
        f = dbg["feats"][l - 2].permute(0, 2, 3, 1).numpy()
        assert np.abs(f[:, ::4, ::4, ::16] - g[f"P{l}_sub"]).max() < 1e-4
    assert np.abs(out[0]["masks28"][:4, 0].numpy() - g["masks28_first4"][0]).max() < 1e-5


def _old_resnet50_fpn(sd, x):
    """the trunk as ONE function, as oracle.mask_rcnn.resnet50_fpn was written before it was split into stem / stages / fpn"""
    import torch.nn.functional as F

    from oracle import mask_rcnn as om

    B = "backbone.body."
    x = F.relu(om._bn(sd, B + "bn1", F.conv2d(x, sd[B + "conv1.weight"], stride=2, padding=3)))
    x = F.max_pool2d(x, 3, 2, 1)
    feats = []
    for li, n in enumerate(om.RESNET50_BLOCKS):
        for bi in range(n):
            P = f"{B}layer{li + 1}.{bi}."
            stride = 2 if (bi == 0 and li > 0) else 1
            idn = x
            o = F.relu(om._bn(sd, P + "bn1", F.conv2d(x, sd[P + "conv1.weight"])))
            o = F.relu(om._bn(sd, P + "bn2", F.conv2d(o, sd[P + "conv2.weight"], stride=stride, padding=1)))
            o = om._bn(sd, P + "bn3", F.conv2d(o, sd[P + "conv3.weight"]))
            if bi == 0:
                idn = om._bn(sd, P + "downsample.1", F.conv2d(x, sd[P + "downsample.0.weight"], stride=stride))
            x = F.relu(o + idn)
        feats.append(x)
    F_ = "backbone.fpn."
    last = F.conv2d(feats[3], sd[F_ + "inner_blocks.3.weight"], sd[F_ + "inner_blocks.3.bias"])
    outs = [F.conv2d(last, sd[F_ + "layer_blocks.3.weight"], sd[F_ + "layer_blocks.3.bias"], padding=1)]
    for i in (2, 1, 0):
        lat = F.conv2d(feats[i], sd[F_ + f"inner_blocks.{i}.weight"], sd[F_ + f"inner_blocks.{i}.bias"])
        last = lat + F.interpolate(last, size=lat.shape[-2:], mode="nearest")
        outs.insert(0, F.conv2d(last, sd[F_ + f"layer_blocks.{i}.weight"], sd[F_ + f"layer_blocks.{i}.bias"], padding=1))
    outs.append(F.max_pool2d(outs[-1], 1, 2, 0))
    return outs, feats


def test_split_trunk_equals_the_one_piece_composition_bit_for_bit():
    """resnet_stem, resnet_stage and fpn, called one by one (as the stage tests do), and resnet50_fpn that composes them give the
    bits of the unsplit trunk in float32; 1 x 64 x 96 is the smallest frame of the stage tests (P5 2 x 3, P6 1 x 2)"""
    from oracle import mask_rcnn as om

    sd = om.synthetic_state_dict(2)
    for n, h, w in ((1, 64, 96), (2, 96, 128)):
        batch, _, _ = om.transform_images(list(om.synthetic_images(n, h, w)), h, w)
        with torch.no_grad():
            ref, ref_c = _old_resnet50_fpn(sd, batch)
            got = om.resnet50_fpn(sd, batch)
            x = om.resnet_stem(sd, batch)
            cs = []
            for li in range(4):
                x = om.resnet_stage(sd, x, li)
                cs.append(x)
            parts = om.fpn(sd, cs)
        Hp, Wp = batch.shape[2:]
        assert [tuple(t.shape) for t in got] == [(n, 256, Hp >> k, Wp >> k) for k in (2, 3, 4, 5)] + [(n, 256, ((Hp >> 5) + 1) // 2, ((Wp >> 5) + 1) // 2)]
        assert all(torch.equal(a, b) for a, b in zip(cs, ref_c))
        assert all(torch.equal(a, b) for a, b in zip(got, ref)) and all(torch.equal(a, b) for a, b in zip(parts, ref))


def test_mask_branch_runs_in_float64_and_agrees_with_float32_to_round_off():
    """mask_branch casts the (float32) RoIAlign output to the weights' dtype, as box_branch does: with float64 weights it runs, and
    the float32 branch differs from it by round-off.  mask_head_logits is the same chain before the sigmoid and the class selection.
    Bound: the logits come from six layers of <= 2304-term float32 dot products of O(1) terms: 1e-5 of the scale is ~100 ulp, an order
    above what sequential-sum round-off gives there and four orders below a wrong weight or pixel (the probabilities' slope is <= 1/4)."""
    from oracle import mask_rcnn as om

    C = 3
    sd = om.synthetic_state_dict(C)
    sd64 = {k: v.double() for k, v in sd.items()}
    g = torch.Generator().manual_seed(3)
    feats = [torch.randn(2, 256, 64 >> k, 96 >> k, generator=g) for k in range(4)]
    sizes = [(250, 380), (256, 384)]
    boxes = [torch.tensor([[10.0, 20.0, 200.0, 240.0], [300.0, 5.0, 330.0, 40.0], [0.0, 0.0, 384.0, 256.0]]), torch.tensor([[50.0, 60.0, 50.0, 90.0]])]
    dets = [dict(boxes=b, labels=torch.tensor([1, 2, 1][: len(b)])) for b in boxes]
    with torch.no_grad():
        m32 = om.mask_branch(sd, feats, dets, sizes)
        m64 = om.mask_branch(sd64, [f.double() for f in feats], dets, sizes)
        roi = om.multiscale_roi_align(feats, boxes, sizes, 14)
        l32, l64 = om.mask_head_logits(sd, roi), om.mask_head_logits(sd64, roi.double())
    assert [tuple(m.shape) for m in m64] == [(3, 1, 28, 28), (1, 1, 28, 28)] and m64[0].dtype == torch.float64 and m32[0].dtype == torch.float32
    assert l64.shape == (4, C, 28, 28) and l64.dtype == torch.float64
    lab = torch.tensor([1, 2, 1, 1])
    assert torch.equal(torch.cat(m32), l32.sigmoid()[torch.arange(4), lab][:, None])   # mask_branch = sigmoid + selection of these logits
    assert torch.equal(torch.cat(m64), l64.sigmoid()[torch.arange(4), lab][:, None])
    scale = max(1.0, l64.abs().max().item())
    err_l = (l32.double() - l64).abs().max().item() / scale
    err_p = (torch.cat(m32).double() - torch.cat(m64)).abs().max().item()
    print(f"[mask_branch] float32 vs float64: logits {err_l:.3e} of scale {scale:.2f}, probabilities {err_p:.3e}")
    assert err_l < 1e-5 and err_p < 2.5e-6, (err_l, err_p)
    assert l64.abs().max() > 0.1   # (not a comparison of zeros)


def test_float64_roi_align_reference_equals_the_oracles_to_round_off():
    """tests/support/detector.py multiscale_roi_align_f64 against oracle.mask_rcnn.multiscale_roi_align (float32, torchvision's
    operation order) on random maps: same level for every box, values within float32 round-off.  Bound: an output is the mean of 4
    samples of 4 products each, accumulated in float32: <= 16 products, 16 additions and a division, each rounded to half an ulp of at
    most max|map| -> 33 * 2^-24 * max|map|."""
    from oracle import mask_rcnn as om
    from oracle import thirdparty as tp
    from tests.support import detector as sup

    g = torch.Generator().manual_seed(11)
    n, Hp, Wp = 2, 128, 160
    feats = [torch.randn(n, 16, Hp >> k, Wp >> k, generator=g) for k in (2, 3, 4, 5)]
    sizes = [(120, 150), (128, 160)]
    special = torch.tensor([
        [40.0, 30.0, 40.0, 90.0],        # zero width: max(roi_w, 1)
        [20.0, 70.0, 100.0, 70.0],       # zero height
        [-300.0, -200.0, -100.0, -90.0],  # wholly outside: every sample is skipped
        [100.0, 90.0, 420.0, 380.0],     # runs past the right / bottom edge
        [-50.0, -40.0, 60.0, 50.0],      # starts before the frame
        [0.0, 0.0, 112.0, 112.0], [10.0, 0.0, 66.0, 224.0],      # sqrt(area) = 112 exactly -> level 3
        [0.0, 0.0, 224.0, 224.0], [0.0, 8.0, 112.0, 456.0],      # 224 -> 4
        [0.0, 0.0, 448.0, 448.0], [-100.0, 0.0, 796.0, 224.0],   # 448 -> 5
        [0.0, 0.0, 111.99, 112.0], [0.0, 0.0, 223.99, 224.0], [0.0, 0.0, 447.99, 448.0],   # just below each threshold
    ])
    xy = torch.rand(40, 2, generator=g) * torch.tensor([150.0, 120.0])
    wh = torch.exp(torch.rand(40, 2, generator=g) * 5.5)   # 1 .. 245 px
    boxes = [torch.cat([special, torch.cat([xy[:20], xy[:20] + wh[:20]], 1)]), torch.cat([special.flip(0), torch.cat([xy[20:], xy[20:] + wh[20:]], 1)])]
    all_boxes = torch.cat(boxes)
    bidx = torch.cat([torch.full((len(b),), float(i)) for i, b in enumerate(boxes)])
    for P in (7, 14):
        ref = om.multiscale_roi_align(feats, boxes, sizes, P)                                     # [K, c, P, P] float32
        got, lv = sup.multiscale_roi_align_f64([f.permute(0, 2, 3, 1) for f in feats], boxes, sizes, P, chunk_bytes=1 << 20)   # (several chunks)
        assert got.dtype == torch.float64 and got.shape == (len(all_boxes), P, P, 16)
        assert lv[: len(special)].tolist() == [2, 2, 3, 4, 2, 3, 3, 4, 4, 5, 5, 2, 3, 4] and set(lv.tolist()) == {2, 3, 4, 5}
        # the oracle's row of every box is RoIAlign on the level chosen here, bit for bit: the same level
        for k in range(len(all_boxes)):
            l = int(lv[k]) - 2
            one = tp.roi_align(feats[l], torch.cat([bidx[k : k + 1, None], all_boxes[k : k + 1]], 1), (P, P), spatial_scale=1.0 / (4 << l), sampling_ratio=2)
            assert torch.equal(one[0], ref[k]), k
        err = (got.permute(0, 3, 1, 2) - ref.double()).abs().max().item()
        bound = 33 * 2.0 ** -24 * max(f.abs().max().item() for f in feats)
        print(f"[roi_align_f64] P {P}: err {err:.3e} (bound {bound:.3e})")
        assert err <= bound, (P, err, bound)
        assert (got[2] == 0).all() and (ref[2] == 0).all()   # the box outside the frame
        assert got[0].abs().max() > 0 and got[1].abs().max() > 0


def test_native_checker_generates_the_oracles_synthetic_network(tmp_path):
    """scripts/microbench/native_detector_check.cpp (the torch-free parity runner used on the GPU box) regenerates weights and images
    from the same hash as oracle.mask_rcnn.synthetic_*: its --checksums mode (host only) must agree tensor by tensor, bit for bit"""
    import shutil
    import subprocess

    root = Path(__file__).resolve().parent.parent
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not Path(hipcc).is_file() or not (root / "megapose6d_amd" / "libmp_engine.so").is_file():
        pytest.skip("needs hipcc and the built engine library")
    from oracle import mask_rcnn as om

    exe = tmp_path / "native_detector_check"
    subprocess.run([hipcc, "-O1", "-std=c++17", "--offload-arch=gfx950", f"-I{root / 'include'}", str(root / "scripts/microbench/native_detector_check.cpp"),
                    "-o", str(exe), f"-L{root / 'megapose6d_amd'}", "-lmp_engine", f"-Wl,-rpath,{root / 'megapose6d_amd'}"], check=True, timeout=300)
    lines = subprocess.run([str(exe), "--checksums", "4"], check=True, capture_output=True, text=True, timeout=300).stdout.split("\n")
    rows = [l.split() for l in lines if l.strip()]

    def ck(a):
        b = np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32).astype(np.uint64)
        k = (np.arange(b.size, dtype=np.uint64) % np.uint64(251)) + np.uint64(1)
        with np.errstate(over="ignore"):
            return int((b * k).sum(dtype=np.uint64))

    spec = om.state_spec(4)
    assert len(rows) == len(spec) + 1
    for (name, shape), row in zip(spec, rows):
        v = om.synthetic_tensor(name, shape)
        assert row[0] == name and int(row[1]) == v.size and int(row[2]) == ck(v), name
    assert int(rows[-1][2]) == ck(om.synthetic_images(1, 24, 32).numpy())
