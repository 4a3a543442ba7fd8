"""CPU: the Python layer of onboarding (megapose6d_amd/onboarding.py, mesh_io.write_ply) where it needs no device -- the PLY round trip,
the bounds `volume_for_views` picks on the analytic sphere's views, and the refusals of `reconstruct_object` and `TsdfVolume`."""
import numpy as np
import pytest
import torch

from megapose6d_amd import mesh_io, onboarding
from tests.support import tsdf as st


def _views_t():
    v = st.sphere_views()
    return dict(depth=torch.from_numpy(v["depth"]), K=torch.from_numpy(v["K"]), TCO=torch.from_numpy(v["TCO"]), masks=torch.from_numpy(v["masks"]),
                rgb=torch.from_numpy(v["rgb"]))


@pytest.mark.parametrize("with_colors,with_normals", [(True, True), (True, False), (False, True), (False, False)])
def test_write_ply_read_ply_round_trip(tmp_path, with_colors, with_normals):
    vol, g = st.corner_volume()
    v, _, f = st.emul_extract(vol, g)
    rng = np.random.RandomState(0)
    v = (v + rng.uniform(-0.1, 0.1, v.shape)).astype(np.float32)
    colors = rng.randint(0, 256, v.shape).astype(np.uint8) if with_colors else None
    normals = mesh_io.vertex_normals(v, f).astype(np.float32) if with_normals else None
    path = mesh_io.write_ply(tmp_path / "m.ply", v, f, colors=None if colors is None else colors / 255.0, normals=normals)
    back = mesh_io.read_ply(path)
    assert back["vertices"].dtype == np.float64 and np.array_equal(back["vertices"].astype(np.float32), v)
    assert back["faces"].dtype == np.int32 and np.array_equal(back["faces"], f)
    assert (back["colors"] is None) == (not with_colors) and (back["normals"] is None) == (not with_normals)
    if with_colors:
        assert np.array_equal(np.rint(back["colors"] * 255).astype(np.uint8), colors)
        again = mesh_io.write_ply(tmp_path / "m8.ply", v, f, colors=colors, normals=normals)           # uint8 colours as they are
        assert again.read_bytes() == path.read_bytes()
    if with_normals:
        assert np.array_equal(back["normals"].astype(np.float32), normals)
    assert back["uvs"] is None and back["texture_path"] is None
    empty = mesh_io.read_ply(mesh_io.write_ply(tmp_path / "e.ply", np.zeros((0, 3)), np.zeros((0, 3), int)))
    assert empty["vertices"].shape == (0, 3) and empty["faces"].shape == (0, 3)
    with pytest.raises(ValueError, match="outside"):
        mesh_io.write_ply(tmp_path / "bad.ply", v, [[0, 1, len(v)]])


def test_volume_for_views_bounds_the_sphere():
    t = _views_t()
    for resolution, margin in ((32, 4), (24, 2), (128, 4)):
        origin, voxel, dims = onboarding.volume_for_views(t["depth"], t["K"], t["TCO"], t["masks"], resolution=resolution, margin_voxels=margin)
        # the eight views see the sphere's extreme points along every axis to within a pixel's footprint (0.4 m / 200 px = 2 mm)
        side = voxel * (resolution - 1 - 2 * margin)
        assert 2 * st.SPHERE_R - 0.004 < side <= 2 * st.SPHERE_R + 1e-6
        assert max(dims) == resolution and all(resolution - 2 <= d <= resolution for d in dims)
        for c in range(3):
            lo, hi = origin[c] + margin * voxel, origin[c] + (dims[c] - 1 - margin) * voxel
            assert -st.SPHERE_R - 1e-6 <= lo < -st.SPHERE_R + 0.002 and st.SPHERE_R - 0.002 - voxel < hi < st.SPHERE_R + voxel
    # without masks the measured pixels are the same here (the background holds no depth)
    assert onboarding.volume_for_views(t["depth"], t["K"], t["TCO"], None, 32) == onboarding.volume_for_views(t["depth"], t["K"], t["TCO"], t["masks"], 32)
    with pytest.raises(ValueError, match="no view holds"):
        onboarding.volume_for_views(t["depth"], t["K"], t["TCO"], torch.zeros_like(t["masks"]))
    with pytest.raises(ValueError, match="resolution"):
        onboarding.volume_for_views(t["depth"], t["K"], t["TCO"], t["masks"], resolution=8, margin_voxels=4)


def test_refusals_that_need_no_device(tmp_path):
    t = _views_t()
    rec = lambda **kw: onboarding.reconstruct_object("obj", **{**dict(depth=t["depth"], K=t["K"], TCO=t["TCO"], out_dir=tmp_path), **kw})   # noqa: E731
    with pytest.raises(ValueError, match=r"depth must be \[n,h,w\]"):
        rec(depth=t["depth"][0])
    with pytest.raises(ValueError, match="at least one view"):
        rec(depth=t["depth"][:0], K=t["K"][:0], TCO=t["TCO"][:0])
    with pytest.raises(ValueError, match="K must be"):
        rec(K=t["K"][:3])
    with pytest.raises(ValueError, match="TCO"):
        rec(TCO=t["TCO"][:, :3])
    K = t["K"].clone()
    K[2, 0, 0] = float("nan")
    with pytest.raises(ValueError, match="not finite"):
        rec(K=K)
    with pytest.raises(ValueError, match="masks must be"):
        rec(masks=t["masks"][:, :10])
    with pytest.raises(ValueError, match="rgb must be"):
        rec(rgb=t["rgb"][..., :2])
    with pytest.raises(ValueError, match="no view holds a measured pixel"):
        rec(masks=torch.zeros_like(t["masks"]))
    with pytest.raises(ValueError, match="no view holds a measured pixel"):
        rec(depth=torch.full_like(t["depth"], float("nan")))
    assert not list(tmp_path.iterdir())
    for bad in (dict(dims=(1, 8, 8)), dict(dims=(8, 513, 8)), dict(dims=(512, 512, 1024)), dict(voxel_size=0.0), dict(voxel_size=float("nan")),
                dict(origin=(0.0, float("inf"), 0.0)), dict(trunc_voxels=0.0), dict(dims=(8, 8))):
        with pytest.raises(ValueError):
            onboarding.TsdfVolume(**{**dict(origin=(0.0, 0.0, 0.0), voxel_size=0.01, dims=(8, 8, 8)), **bad})
